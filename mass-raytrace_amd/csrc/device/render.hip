// render.hip — the wavefront path-tracing integrator for gfx950.
//
// Replaces render()'s per-thread pixel loop (main.rs:235-290): each sample
// (one camera path, main.rs:257-263) becomes a path slot in a pool of SoA
// HBM buffers, advanced one segment per iteration by two kernels:
//   k_trace : closest hit of every active ray (World::intersect; trace.hip) [k2]
//   k_shade : emit/scatter/background, path termination and wave
//             ballot/prefix-sum compaction of the survivors           [k3,k4]
//   k_reserve + k_refill : new camera rays (Camera::ray) for the free
//             slots behind the survivors                              [k1]
// Finished samples are written to a per-(pixel,sample) result slab and folded
// into the caller's accumulation buffers in sample order by k_accumulate [k5]
// (Image::merge, main.rs:629-638), so the sums do not depend on scheduling
// or on how tiles are sharded across GPUs.
#include <algorithm>
#include <mutex>

#include "ctx.h"
#include "shade.h"

using namespace mrt;

namespace {

// k_shade's workgroup: its survivors are grouped (option shade_bin) within
// one workgroup, so the size sets the grouping's scope
#ifndef MRT_SHADE_BLOCK
#define MRT_SHADE_BLOCK 256
#endif
constexpr int kShadeBlock = MRT_SHADE_BLOCK;

__device__ __forceinline__ void gen_work(const DevCamera& cam, const RenderParams& rp, uint32_t g, float4& ro,
                                         float4& rd, uint4& rs) {
  // work items run sample-minor: the samples of one pixel are consecutive
  // (camera rays of a wave nearly equal), and the results slab is laid out
  // the same way, g = pixel * spp + sample
  uint32_t lp = g / rp.spp;
  uint32_t s_local = g - lp * rp.spp;
  uint32_t p = rp.pixlist[lp];  // lp < n_pix by construction (g < G)
  uint32_t y = p / rp.W, x = p - y * rp.W;
  PathRng rng = path_rng(rp.seed, p, rp.sample_base + s_local);
  V3 o, d;
  camera_ray(cam, x, y, rp.W, rp.H, rng, o, d);
  ro = make_float4(o.x, o.y, o.z, __uint_as_float(g));
  rd = make_float4(d.x, d.y, d.z, __uint_as_float(0u));
  rs = rng_pack(rng);
}

// Initial pool: work items [base, base + n0) into slots [0, n0).
__global__ __launch_bounds__(kBlock) void k_generate(DevCamera cam, RenderParams rp, PathBufs out, uint32_t base,
                                                     uint32_t n0) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n0) return;
  float4 ro, rd;
  uint4 rs;
  gen_work(cam, rp, base + i, ro, rd, rs);
  out.ro[i] = ro;
  out.rd[i] = rd;
  out.thr[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);  // L = 0: rad not written
  out.rng[i] = rs;
}

// Lagged status read of a queue (host loop, one per batch): the fields the
// host needs, written by one wave straight into pinned host memory. A
// hipMemcpyAsync to pinned memory ran as a 1024-thread blit kernel, which
// waited for a CU with 16 free wave slots while both queues' kernels held
// the chip (12-46 ms per read in the kernel trace, the queue's stream stalled
// behind it); one wave finds a slot at once.
__global__ void k_status(const Ctrl* ctrl, const uint32_t* work, HostStatus* out) {
  if (threadIdx.x != 0) return;
  HostStatus h;
  h.active0 = ctrl->active[0];
  h.active1 = ctrl->active[1];
  h.shade_short = ctrl->shade_short;
  h.work = *work;
  *out = h;
  __threadfence_system();
}

// Refill after k_shade compacted the survivors of pool `cur` into the next
// pool (ctrl->active[cur ^ 1] of them): reserve work items for the free slots
// behind them from the shared work counter. One thread; the counter is only
// advanced while it is below G, so it passes G by at most a pool per queue.
__global__ void k_reserve(Ctrl* ctrl, uint32_t cur, uint32_t* work, uint32_t G, uint32_t cap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long sv = ctrl->surv[cur ^ 1];  // 0 unless shade_bin 2
  const uint32_t lo = ctrl->active[cur ^ 1] + (uint32_t)sv, hi = (uint32_t)(sv >> 32), n = lo + hi;
  const uint32_t want = n < cap ? cap - n : 0u;
  uint32_t m = 0, base = G;
  if (want && __hip_atomic_load(work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < G) {
    base = atomicAdd(work, want);
    m = base < G ? (G - base < want ? G - base : want) : 0u;
  }
  ctrl->gen_slot = lo;
  ctrl->gen_count = m;
  ctrl->gen_base = base;
  // the top block [cap - hi, cap) closes onto the refill's end lo + m: its
  // paths at or past the new end E move into the free slots below E
  const uint32_t E = n + m, g = cap - E;
  const uint32_t mv = g < hi ? g : hi;
  ctrl->gen_move = mv;
  ctrl->gen_move_src = cap - mv;
  ctrl->gen_move_dst = lo + m;
  ctrl->active[cur ^ 1] = E;
  ctrl->surv[cur ^ 1] = 0;
}

// ... and generate them (camera rays of consecutive work items, i.e. pixel
// order): the next k_trace finds the new paths together behind the
// survivors instead of scattered among them one per finished slot.
__global__ __launch_bounds__(kBlock) void k_refill(DevCamera cam, RenderParams rp, PathBufs out, const Ctrl* ctrl) {
  const uint32_t m = ctrl->gen_count, slot = ctrl->gen_slot, base = ctrl->gen_base;
  const uint32_t mv = ctrl->gen_move, src = ctrl->gen_move_src, dst = ctrl->gen_move_dst;
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < mv; j += gridDim.x * kBlock) {
    // sources [cap - mv, cap) and destinations [lo + m, lo + m + mv) are disjoint
    const uint32_t a = src + j, b = dst + j;
    const float4 thr = out.thr[a], ro = out.ro[a], rd = out.rd[a];
    const uint4 rs = out.rng[a];
    out.ro[b] = ro;
    out.rd[b] = rd;
    out.thr[b] = thr;
    out.rng[b] = rs;
    if (holds_l(thr)) out.rad[b] = out.rad[a];
  }
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock) {
    float4 ro, rd;
    uint4 rs;
    gen_work(cam, rp, base + j, ro, rd, rs);
    const uint32_t i = slot + j;
    out.ro[i] = ro;
    out.rd[i] = rd;
    out.thr[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);  // L = 0: rad not written
    out.rng[i] = rs;
  }
}

// k_shade only shades and compacts: new camera rays go in behind the
// survivors (k_reserve + k_refill). (Round 3's in-place regeneration of
// finished slots is profiles/r3_experiments/ab_branches.patch.)
// WPE: waves per SIMD the register budget is sized for (8: 64 VGPRs, 16 B of
// scratch; 7: 68 VGPRs, none). With 8, k_shade takes more of the CU beside
// the other queue's k_trace; a world whose records stream from the Infinity
// Cache runs better with 7 (mesh_ply 948.6 -> 969.0, 6: 962.9 Msamples/s),
// an L2-resident one with 8 (sphere_grid 808.8, 7: 778.1, 6: 761.0;
// profiles/r3_tune2/wpe.txt).
template <bool COUNT, bool EXT, int WPE>
__global__ __launch_bounds__(kShadeBlock, WPE) void k_shade(DevScene S, RenderParams rp, PathBufs in, PathBufs out,
                                                  const uint4* hits, Ctrl* ctrl, uint32_t cur, float4* results,
                                                  DevCounters* cnt) {
  const uint32_t n = ctrl->active[cur];
  if (blockIdx.x == 0 && threadIdx.x < kGroups) ctrl->group_next[threadIdx.x * 32] = 0;  // next k_trace
  // one workgroup per 256 live paths: the host sizes the grid from a bound on
  // the live count (shade_grid), so a drain launch does not dispatch a
  // workgroup per 256 slots of the whole pool. A bound that fell short is
  // reported to the host, never dropped silently. (A grid-stride loop here
  // made the kernel spill 80 B instead of 44 and cost 3.5% of the frame.)
  if (blockIdx.x == 0 && threadIdx.x == 0 && n > gridDim.x * kShadeBlock) ctrl->shade_short = n;
  LocalCounters lc;
  uint32_t nbounce = 0, nsample = 0, nshaded = 0;
  __shared__ uint32_t s_cnt[kShadeBlock / 64], s_base, s_hist[kOutKeys];
  const uint32_t wave = threadIdx.x / 64;
  {
    const uint32_t base = blockIdx.x * kShadeBlock;
    if (base >= n) return;
    const uint32_t i = base + threadIdx.x;
    bool alive = false;
    float4 ro{}, rd{}, thr{}, rad{};
    uint4 rs{};
    uint32_t mat = kShadeIdle, mkind = 0;
    if (i < n) {
      nshaded += 1;
      // the lane's own slot in one batch, the hit first: the primitive's
      // gather goes out on it while the state is still in flight
      const uint4 hv = hits[i];
      thr = in.thr[i];
      ro = in.ro[i];
      rd = in.rd[i];
      rs = in.rng[i];
      if (holds_l(thr)) rad = in.rad[i];
      Hit h{__uint_as_float(hv.x), hv.y, hv.z};
      V3 o{ro.x, ro.y, ro.z}, d{rd.x, rd.y, rd.z}, T{thr.x, thr.y, thr.z}, L{rad.x, rad.y, rad.z};
      uint32_t g = __float_as_uint(ro.w), k = __float_as_uint(rd.w);
      PathRng rng = rng_unpack(rs);
      const bool cont = shade_step<EXT>(S, rp.max_depth, h, o, d, T, L, k, rng, lc, nbounce, mat, mkind);
      if (cont) {
        alive = true;
        ro = make_float4(o.x, o.y, o.z, __uint_as_float(g));
        rd = make_float4(d.x, d.y, d.z, __uint_as_float(k));
        thr = make_float4(T.x, T.y, T.z, __uint_as_float(nonzero_bits(L.x, L.y, L.z) ? kHoldsL : 0u));
        rad = make_float4(L.x, L.y, L.z, 0.0f);
        rs = rng_pack(rng);
      } else {
#ifndef MRT_PROBE_NO_RESULTS  // probe build (tools/shade_probe.sh): k_shade's HBM writes without the scattered results stores
        results[MRT_IDX(S, g, rp.G, 21)] = make_float4(L.x, L.y, L.z, __uint_as_float(k));
#endif
        nsample += 1;
      }
    }
    if (COUNT) shade_coherence(mat, mkind, lc);
    // compact the survivors into the next pool: one atomic per workgroup
    // (same-address atomics from every wave serialise in L2)
    uint32_t slot;
    if (rp.shade_bin) {  // survivors grouped by the material kind they scattered from (wg_reserve_keyed)
      // key: the material kind scattered from (the hit's own record's, as
      // shade_step read it: no load here) and the signs of the new ray's y and x
      const uint32_t kind = alive ? (mkind & 7u) : 0u;
      if (rp.shade_bin == 2) {  // y sign: the two ends of the pool; kind and x, z signs within
        const uint32_t key = (rd.y < 0.0f ? 32u : 0u) + kind * 4u + (rd.x < 0.0f ? 2u : 0u) + (rd.z < 0.0f ? 1u : 0u);
        slot = wg_reserve_keyed(&ctrl->active[cur ^ 1], alive, key, s_hist, &ctrl->surv[cur ^ 1], rp.pool_cap);
      } else {
        const uint32_t key = kind * 4u + (rd.y < 0.0f ? 2u : 0u) + (rd.x < 0.0f ? 1u : 0u);
        slot = wg_reserve_keyed(&ctrl->active[cur ^ 1], alive, key, s_hist);
      }
    } else {
      const unsigned long long alive_mask = __ballot(alive);
      slot = wg_reserve<kShadeBlock / 64>(&ctrl->active[cur ^ 1], (uint32_t)__popcll(alive_mask), wave, s_cnt, s_base) +
             lane_rank(alive_mask);
    }
    if (alive) {
      uint32_t pos = MRT_IDX(S, slot, rp.pool_cap, 22);
      out.ro[pos] = ro;
      out.rd[pos] = rd;
      out.thr[pos] = thr;
      if (holds_l(thr)) out.rad[pos] = rad;
      out.rng[pos] = rs;
    }
  }
  if (COUNT) flush_counters(cnt, lc, 0, 0, nsample, nbounce, nshaded);
}

// The whole path loop in one persistent kernel: every lane owns a path
// (work item g = pixel*spp + sample, gen_work), steps its closest-hit traversal like
// k_trace, and when a segment ends shades it in place (shade_step) and
// continues with the scattered ray — no pool buffers, no per-bounce launch
// and no per-launch tail. Finished paths write results[g] (accumulated in
// sample order by k_accumulate, so the image is independent of scheduling);
// idle lanes take new work items from ctrl->next_work. slot_ro/slot_rd hold
// each lane's current world ray (re-read when leaving an instance and when
// shading, instead of keeping it in registers).
//
// ADOPT (the wavefront loop's drain, "finish"): instead of new work items the
// lanes adopt the paths of a wavefront pool (`pool`, ctrl->active[cur] of
// them, handed out by ctrl->next_work) in the state k_shade left them — the
// next ray to trace, T, L, bounces, RNG — and run each to its end. The
// wavefront loop switches to it once its work counter is exhausted and few
// paths remain: every per-bounce k_trace launch lasts at least as long as its
// slowest ray (mesh_ply: ~2 ms), so a pool draining over ~50 bounces pays that
// floor ~50 times, while here a lane moves on to its path's next segment as
// soon as its own segment ends.
template <bool COUNT, bool ALPHA, bool ADOPT>
__global__ __launch_bounds__(kBlock) void k_render(DevScene S, DevCamera cam, RenderParams rp, float4* slot_ro,
                                                   float4* slot_rd, Ctrl* ctrl, float4* results, DevCounters* cnt,
                                                   TraceTune tune, PathBufs pool, uint32_t cur) {
  const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t n_src = ADOPT ? ctrl->active[cur] : rp.G;  // uniform
  const TravIn tin{S, reinterpret_cast<const uint4*>(S.slots), S.world_begin, slot_ro, slot_rd, kTmin};
  LocalCounters lc;
  uint32_t seg = 0, nh = 0, nsamples = 0, nbounces = 0;
  Trav t{};
  t.done = true;
  t.ray = slot;
  uint32_t g = kIdle, k = 0;
  V3 T{0, 0, 0}, L{0, 0, 0};
  PathRng rng{0, 0};
  bool drained = false;  // wave-uniform: the work counter passed G
  for (;;) {
    const unsigned long long idle = __ballot(g == kIdle);
    const uint32_t n_idle = (uint32_t)__popcll(idle);
    if (!drained && (n_idle >= tune.refill || n_idle == 64)) {
      uint32_t b = 0;
      if (lane_id() == 0) b = atomicAdd(&ctrl->next_work, n_idle);
      b = __shfl(b, 0, 64);
      drained = b + n_idle >= n_src;
      if (g == kIdle) {
        const uint32_t w = b + lane_rank(idle);
        if (w < n_src) {
          float4 ro, rd;
          uint4 rs;
          if (ADOPT) {  // a wavefront path: {o, g} {d, bounces} T L rng (PathBufs)
            const float4 tv = pool.thr[w];  // one batch; rad, rare, behind it
            ro = pool.ro[w];
            rd = pool.rd[w];
            rs = pool.rng[w];
            const float4 lv = holds_l(tv) ? pool.rad[w] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            g = __float_as_uint(ro.w);
            k = __float_as_uint(rd.w);
            T = V3{tv.x, tv.y, tv.z};
            L = V3{lv.x, lv.y, lv.z};
          } else {
            gen_work(cam, rp, w, ro, rd, rs);
            g = w;
            k = 0;
            T = V3{1.0f, 1.0f, 1.0f};
            L = V3{0.0f, 0.0f, 0.0f};
          }
          rng = rng_unpack(rs);
          slot_ro[slot] = ro;
          slot_rd[slot] = rd;
          trav_init(tin, t, slot, INFINITY);
        }
      }
    }
    if (drained && __ballot(g != kIdle) == 0) break;
    // one traversal step (as k_trace)
    const bool busy = g != kIdle && !t.done;
    const bool at_box = busy && trav_at_box(t);
    const unsigned long long box_mask = __ballot(at_box);
    const unsigned long long prim_mask = __ballot(busy && !at_box);
    if (at_box) trav_box<COUNT>(tin, t, lc);
    if ((__popcll(prim_mask) >= tune.prim_batch || box_mask == 0) && busy && !at_box)
      trav_prim<COUNT, ALPHA>(tin, t, lc);
    // shade finished segments once enough lanes wait (or nothing else runs)
    const bool ready = g != kIdle && t.done;
    const unsigned long long ready_mask = __ballot(ready);
    if (ready_mask != 0 && ((uint32_t)__popcll(ready_mask) >= tune.shade_batch || (box_mask | prim_mask) == 0)) {
      if (ready) {
        const Hit h = trav_hit(tin, t);
        seg += 1;
        nh += h.prim != kRefNone;
        const float4 o4 = slot_ro[slot], d4 = slot_rd[slot];
        V3 o{o4.x, o4.y, o4.z}, d{d4.x, d4.y, d4.z};
        uint32_t mat, mkind;
        if (shade_step<false>(S, rp.max_depth, h, o, d, T, L, k, rng, lc, nbounces, mat, mkind)) {
          slot_ro[slot] = make_float4(o.x, o.y, o.z, 0.0f);
          slot_rd[slot] = make_float4(d.x, d.y, d.z, 0.0f);
          trav_init(tin, t, slot, INFINITY);
        } else {
          results[MRT_IDX(S, g, rp.G, 21)] = make_float4(L.x, L.y, L.z, __uint_as_float(k));
          nsamples += 1;
          g = kIdle;
        }
      }
    }
  }
  if (COUNT) flush_counters(cnt, lc, seg, nh, nsamples, nbounces);
}

// Image::merge in sample order: acc = ((acc + s0) + s1) + ...
// A workgroup sums kAccPix pixels: blocks of kAccS samples of all of them
// are staged through LDS with coalesced loads (a pixel's samples are
// contiguous in the pixel-major slab), then each of the first kAccPix
// threads adds its pixel's samples in sample order — the same sequence of
// float additions as one thread walking its pixel's samples, so the sums are
// bit-identical, at HBM rate instead of one 16-KiB-strided line per lane.
constexpr uint32_t kAccPix = 64, kAccS = 16, kAccPad = kAccS + 1;  // +1 quad per row: no bank-aligned rows
__global__ __launch_bounds__(kBlock) void k_accumulate(const float4* results, uint32_t n_pix, uint32_t n_samples,
                                                       const uint32_t* pixlist, float* accum_rgb,
                                                       uint32_t* accum_bounces) {
  __shared__ float4 tile[kAccPix * kAccPad];
  const uint32_t lp0 = blockIdx.x * kAccPix;
  const uint32_t n_here = n_pix - lp0 < kAccPix ? n_pix - lp0 : kAccPix;
  const uint32_t j = threadIdx.x;  // the pixel this thread sums (j < n_here)
  float r = 0.0f, g = 0.0f, b = 0.0f;
  uint32_t k = 0, p = 0;
  if (j < n_here) {
    p = pixlist[lp0 + j];
    r = accum_rgb[3 * (size_t)p], g = accum_rgb[3 * (size_t)p + 1], b = accum_rgb[3 * (size_t)p + 2];
    k = accum_bounces[p];
  }
  for (uint32_t s0 = 0; s0 < n_samples; s0 += kAccS) {
    const uint32_t sb = n_samples - s0 < kAccS ? n_samples - s0 : kAccS;
    for (uint32_t e = threadIdx.x; e < kAccPix * kAccS; e += kBlock) {
      const uint32_t px = e / kAccS, sx = e % kAccS;
      if (px < n_here && sx < sb) tile[px * kAccPad + sx] = results[(size_t)(lp0 + px) * n_samples + s0 + sx];
    }
    __syncthreads();
    if (j < n_here) {
      for (uint32_t sx = 0; sx < sb; ++sx) {
        const float4 q = tile[j * kAccPad + sx];
        r = r + q.x;
        g = g + q.y;
        b = b + q.z;
        k += __float_as_uint(q.w);
      }
    }
    __syncthreads();
  }
  if (j < n_here) {
    accum_rgb[3 * (size_t)p] = r;
    accum_rgb[3 * (size_t)p + 1] = g;
    accum_rgb[3 * (size_t)p + 2] = b;
    accum_bounces[p] = k;
  }
}

// The k_shade / k_render variant for a scene and a launch.
using ShadeFn = void (*)(DevScene, RenderParams, PathBufs, PathBufs, const uint4*, Ctrl*, uint32_t, float4*,
                         DevCounters*);
ShadeFn shade_kernel(bool count, bool ext, int wpe) {
  return with_value<true, false>(count, [&](auto COUNT) {
    return with_value<true, false>(ext, [&](auto EXT) {
      return with_value<7, 8>(wpe, [&](auto WPE) -> ShadeFn { return k_shade<COUNT, EXT, WPE>; });
    });
  });
}
using RenderFn = void (*)(DevScene, DevCamera, RenderParams, float4*, float4*, Ctrl*, float4*, DevCounters*,
                          TraceTune, PathBufs, uint32_t);
RenderFn render_kernel(bool count, bool alpha, bool adopt) {
  return with_value<true, false>(count, [&](auto COUNT) {
    return with_value<true, false>(alpha, [&](auto ALPHA) {
      return with_value<true, false>(adopt, [&](auto ADOPT) -> RenderFn { return k_render<COUNT, ALPHA, ADOPT>; });
    });
  });
}

// k_shade's grid for a pool known to hold at most `bound` live paths: one
// workgroup per 256 of them.
// While the work counter has items left the pool refills to capacity; once
// it is exhausted the live count only falls, so the last status the host
// read bounds every later launch — a drain launch then dispatches a few
// workgroups instead of one per 256 slots of the whole pool.
uint32_t shade_grid(const Queue& q, size_t bound) {
  const size_t n = std::min(q.cap, bound);
  return (uint32_t)std::max<size_t>(1, (n + kShadeBlock - 1) / kShadeBlock);
}

// device bytes of a pool of P paths over the context's queues: two state
// sets (5 x 16 B each) + the hit record per path, 256-B aligned sections
constexpr size_t kPathBytes = 16 * (2 * 5 + 1);
size_t pool_bytes(const mrt_ctx* c, size_t P) {
  const size_t K = (size_t)c->tun.queues, per_q = (P + K - 1) / K;
  return (kPathBytes * per_q + 4096) * K;
}

// Sizes a render's path pool and results slab to the device:
// they must fit the memory free now minus mem_reserve, since several
// contexts may share one device (a multi-device context over {0,0,0}, ranks
// rehearsed on one GPU) and the defaults alone ask for ~98 GiB. When either
// buffer has to grow both are released and planned afresh: the pool shrinks
// first (its size barely matters from 128M paths on), down to
// kPoolFloor paths, then the samples per results chunk (more chunks, the
// same image: chunks accumulate in sample order). The planning of the
// contexts of a process is serialised, so each sees the others' buffers.
constexpr size_t kPoolFloor = (size_t)64 << 20;
std::mutex g_alloc_mutex;
void plan_buffers(mrt_ctx* c, uint32_t n_pix, uint32_t& spp_chunk, bool need_pool) {
  std::lock_guard<std::mutex> lock(g_alloc_mutex);
  size_t P = need_pool ? std::min<size_t>((size_t)n_pix * spp_chunk, c->tun.pool_paths) : 0;
  if (P <= c->pool_cap && (size_t)n_pix * spp_chunk <= c->results_cap) return;
  HIP_CHECK(hipDeviceSynchronize());  // the queues may still use the old buffers
  if (c->pool_mem) HIP_CHECK(hipFree(c->pool_mem));
  c->pool_mem = nullptr;
  c->pool_cap = 0;
  if (c->results) HIP_CHECK(hipFree(c->results));
  c->results = nullptr;
  c->results_cap = 0;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const size_t reserve = c->tun.mem_reserve;
  const size_t budget = free_b > reserve ? free_b - reserve : 0;
  for (;;) {
    const size_t need = (P ? pool_bytes(c, P) : 0) + (size_t)n_pix * spp_chunk * 16;
    if (need <= budget) break;
    if (P > kPoolFloor) {
      P = std::max(kPoolFloor, P / 2);
    } else if (spp_chunk > 1) {
      spp_chunk = spp_chunk / 2;
      if (P) P = std::min<size_t>(P, (size_t)n_pix * spp_chunk);
    } else {
      throw ApiError{MRT_ERR_NOMEM, "device memory: " + std::to_string(free_b >> 20) + " MiB free, mem_reserve_mb " +
                                        std::to_string(reserve >> 20) + ": not even one sample per pixel fits"};
    }
  }
  if (P) ensure_pool(c, P);
  HIP_CHECK(hipMalloc(&c->results, (size_t)n_pix * spp_chunk * 16));  // released above
  c->results_cap = (size_t)n_pix * spp_chunk;
}

// One chunk's parameters: `cs` samples per pixel from sample `done` of the
// render `a`, over the shard's pixels.
RenderParams chunk_params(const mrt_ctx* c, const mrt_render_args* a, const uint32_t* pixlist_d, uint32_t n_pix,
                          uint32_t done, uint32_t cs, uint32_t pool_cap) {
  return RenderParams{a->width, a->height, a->seed, a->max_depth, n_pix, /*G*/ n_pix * cs, /*spp*/ cs,
                      /*sample_base*/ a->spp_begin + done, pool_cap, pixlist_d, (uint32_t)c->tun.shade_bin};
}

// The drain hand-off's occupancy grid (each queue has as many lane-ray slots).
uint32_t finish_grid(mrt_ctx* c, bool count) {
  return persistent_grid(c, (const void*)render_kernel(count, c->scene_alpha, true), 0, c->tun.queues > 1);
}

// Finish queue qi's pool bufs[cur] (ctrl->active[cur] paths) with the fused
// kernel in adopt mode; each queue uses its own range of lane-ray slots.
void launch_finish(mrt_ctx* c, int qi, uint32_t cur, const RenderParams& rp, bool count, float4* res) {
  Queue& q = c->q[qi];
  const uint32_t full = finish_grid(c, count);
  const size_t lanes = (size_t)full * kBlock;
  const uint32_t grid = std::max<uint32_t>(c->cus, full / c->tun.finish_grid_div);
  ensure_slots(c, lanes * kMaxQueues);
  float4* sro = c->slot_ro + lanes * qi;
  float4* srd = c->slot_rd + lanes * qi;
  HIP_CHECK(hipMemsetAsync(&q.ctrl->next_work, 0, 4, q.stream));
  hipLaunchKernelGGL(render_kernel(count, c->scene_alpha, true), dim3(grid), dim3(kBlock), 0, q.stream, c->S, c->cam, rp,
                     sro, srd, q.ctrl, res, c->d_cnt, c->tun.trace, q.bufs[cur], cur);
  HIP_CHECK(hipGetLastError());
}

// The fused path loop: one k_render launch + one k_accumulate per chunk.
void render_fused(mrt_ctx* c, const mrt_render_args* a, const uint32_t* pixlist_d, uint32_t n_pix, uint32_t spp_chunk,
                  float* d_rgb, uint32_t* d_b, hipStream_t st) {
  const bool count = (a->flags & MRT_RENDER_COUNTERS) != 0;
  const bool timing = (a->flags & MRT_RENDER_TIME_KERNELS) != 0;
  plan_buffers(c, n_pix, spp_chunk, false);
  wait_queues(c, st);
  for (uint32_t done = 0; done < a->spp_count; done += spp_chunk) {
    const uint32_t cs = std::min(spp_chunk, a->spp_count - done);
    if (a->max_depth == 0) continue;  // trace(ray, 0) returns (0, 0): nothing to add
    const RenderParams rp = chunk_params(c, a, pixlist_d, n_pix, done, cs, 0);
    Ctrl init{{0, 0}, 0, 0};
    HIP_CHECK(hipMemcpyAsync(c->q[0].ctrl, &init, sizeof(Ctrl), hipMemcpyHostToDevice, st));
    if (timing) HIP_CHECK(hipEventRecord(c->tev[0], st));
    const RenderFn f = render_kernel(count, c->scene_alpha, false);
    const uint32_t grid = persistent_grid(c, (const void*)f, 0);
    ensure_slots(c, (size_t)grid * kBlock);
    hipLaunchKernelGGL(f, dim3(grid), dim3(kBlock), 0, st, c->S, c->cam, rp, c->slot_ro, c->slot_rd, c->q[0].ctrl,
                       c->results, c->d_cnt, c->tun.trace, PathBufs{}, 0u);
    HIP_CHECK(hipGetLastError());
    if (timing) {
      HIP_CHECK(hipEventRecord(c->tev[1], st));
      HIP_CHECK(hipEventSynchronize(c->tev[1]));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, c->tev[0], c->tev[1]));
      c->kstats.trace_ms += ms;
      c->kstats.trace_launches++;
      c->kstats.iterations++;
    }
    hipLaunchKernelGGL(k_accumulate, dim3((n_pix + kAccPix - 1) / kAccPix), dim3(kBlock), 0, st, (const float4*)c->results,
                       n_pix, cs, pixlist_d, d_rgb, d_b);
    HIP_CHECK(hipGetLastError());
  }
  mark_ctx_busy(c, st);
}

// pending kernel-timing marks resolved at the start of a timed render once
// this many accumulated (a caller that never reads the stats)
constexpr size_t kMaxPendingMarks = 1u << 14;

}  // namespace

// `st` waits for the wavefront queues' last render (their buffers are reused).
void wait_queues(mrt_ctx* c, hipStream_t st) {
  for (Queue& q : c->q)
    if (q.join) HIP_CHECK(hipStreamWaitEvent(st, q.join, 0));
}

// P paths over the context's queues.
void ensure_pool(mrt_ctx* c, size_t P) {
  if (P <= c->pool_cap) return;
  HIP_CHECK(hipDeviceSynchronize());  // the queues may still be draining into the old pool
  if (c->pool_mem) HIP_CHECK(hipFree(c->pool_mem));
  c->pool_mem = nullptr;
  c->pool_cap = 0;
  const int K = c->tun.queues;
  const size_t per_q = (P + K - 1) / K;
  HIP_CHECK(hipMalloc(&c->pool_mem, pool_bytes(c, P)));
  char* p = (char*)c->pool_mem;
  auto take = [&](size_t bytes) {
    char* r = p;
    p += (bytes + 255) & ~(size_t)255;
    return r;
  };
  for (int k = 0; k < K; ++k) {
    Queue& q = c->q[k];
    for (int b = 0; b < 2; ++b) {
      q.bufs[b].ro = (float4*)take(16 * per_q);
      q.bufs[b].rd = (float4*)take(16 * per_q);
      q.bufs[b].thr = (float4*)take(16 * per_q);
      q.bufs[b].rad = (float4*)take(16 * per_q);
      q.bufs[b].rng = (uint4*)take(16 * per_q);
    }
    q.hits = (uint4*)take(16 * per_q);
    q.cap = per_q;
  }
  c->pool_cap = per_q * K;
}

void ensure_slots(mrt_ctx* c, size_t n) {
  if (n <= c->slots_cap) return;
  if (c->slot_ro) HIP_CHECK(hipDeviceSynchronize());  // a queue set's drain may still use them
  if (c->slot_ro) HIP_CHECK(hipFree(c->slot_ro));
  c->slot_ro = nullptr;
  c->slot_rd = nullptr;
  HIP_CHECK(hipMalloc(&c->slot_ro, 32 * n));
  c->slot_rd = c->slot_ro + n;
  c->slots_cap = n;
}

// MRT_TILE x MRT_TILE tiles in raster order; shard si of sc owns t % sc == si;
// pixels of a tile in raster order, y = 0 the bottom row (main.rs:253-263)
std::vector<uint32_t> shard_pixel_list(uint32_t W, uint32_t H, uint32_t si, uint32_t sc) {
  uint32_t tx = (W + MRT_TILE - 1) / MRT_TILE, ty = (H + MRT_TILE - 1) / MRT_TILE;
  std::vector<uint32_t> list;
  for (uint32_t t = si; t < tx * ty; t += sc) {
    uint32_t bx = (t % tx) * MRT_TILE, by = (t / tx) * MRT_TILE;
    for (uint32_t py = 0; py < MRT_TILE; ++py)
      for (uint32_t px = 0; px < MRT_TILE; ++px) {
        uint32_t x = bx + px, y = by + py;
        if (x < W && y < H) list.push_back(y * W + x);
      }
  }
  return list;
}

std::pair<uint32_t*, uint32_t> pixlist(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc) {
  auto key = std::make_tuple(W, H, si, sc);
  auto it = c->pixlists.find(key);
  if (it != c->pixlists.end()) return it->second;
  const std::vector<uint32_t> list = shard_pixel_list(W, H, si, sc);
  uint32_t* d = nullptr;
  if (!list.empty()) {
    HIP_CHECK(hipMalloc(&d, list.size() * 4));
    HIP_CHECK(hipMemcpy(d, list.data(), list.size() * 4, hipMemcpyHostToDevice));
  }
  auto v = std::make_pair(d, (uint32_t)list.size());
  c->pixlists[key] = v;
  return v;
}

// Work enqueued on a caller's stream `st` that writes the context's shared
// buffers (q[0].ctrl, the results slab, the lane-ray slots): the next
// wavefront render forks its queues after acc_done, so recording it here
// orders that render after this work too.
void mark_ctx_busy(mrt_ctx* c, hipStream_t st) { HIP_CHECK(hipEventRecord(c->acc_done, st)); }

void render_device(mrt_ctx* c, const mrt_render_args* a, float* d_rgb, uint32_t* d_b, hipStream_t st) {
  if (!a) throw ApiError{MRT_ERR_INVALID, "null render args"};
  if (!c->has_scene) throw ApiError{MRT_ERR_STATE, "no scene uploaded"};
  if (!c->has_camera) throw ApiError{MRT_ERR_STATE, "no camera set"};
  if (a->width == 0 || a->height == 0) throw ApiError{MRT_ERR_INVALID, "empty image"};
  if ((uint64_t)a->width * a->height >= (1ull << 32)) throw ApiError{MRT_ERR_INVALID, "image too large"};
  uint32_t sc = a->shard_count ? a->shard_count : 1;
  if (a->shard_index >= sc) throw ApiError{MRT_ERR_INVALID, "shard_index >= shard_count"};
  if (a->spp_count == 0) return;
  if ((uint64_t)a->spp_begin + a->spp_count > 0xFFFFFFFFull) throw ApiError{MRT_ERR_INVALID, "sample index overflow"};
  auto pl = pixlist(c, a->width, a->height, a->shard_index, sc);
  const uint32_t n_pix = pl.second;
  if (n_pix == 0) return;
  const bool count = (a->flags & MRT_RENDER_COUNTERS) != 0;
  const bool simple = (a->flags & MRT_RENDER_SIMPLE_TRACE) != 0;
  const bool scene_rng = c->facts.trav_rng;
  // results slab <= results_max samples (16 B each); pool <= pool_paths
  uint32_t spp_chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(a->spp_count, c->tun.results_max / n_pix));
  if (simple && c->scene_ext)
    throw ApiError{MRT_ERR_INVALID, "MRT_RENDER_SIMPLE_TRACE does not support composite surfaces, CubeMap backgrounds or Eve materials"};
  if ((a->flags & MRT_RENDER_FUSED) && !simple) {
    if (scene_rng)
      throw ApiError{MRT_ERR_INVALID, "MRT_RENDER_FUSED does not support scenes whose traversal draws (Volume, Mix alpha)"};
    if (c->scene_ext)
      throw ApiError{MRT_ERR_INVALID, "MRT_RENDER_FUSED does not support composite surfaces, CubeMap backgrounds or Eve materials"};
    render_fused(c, a, pl.first, n_pix, spp_chunk, d_rgb, d_b, st);
    return;
  }
  plan_buffers(c, n_pix, spp_chunk, true);
  const int K = c->tun.queues;
  const bool timing = (a->flags & MRT_RENDER_TIME_KERNELS) != 0;
  if (timing && c->pend_marks.size() + c->pend_fin.size() > kMaxPendingMarks) resolve_kernel_timing(c);
  // the drain hand-off (launch_finish): the fused kernel has no traversal
  // draws or composite surfaces; its lane-ray slots are allocated here, before
  // any queue runs (ensure_slots reallocates)
  const bool can_finish = !scene_rng && !c->scene_ext && !simple;
  const uint32_t finish_paths = can_finish ? c->tun.finish_paths : 0u;
  if (finish_paths) ensure_slots(c, (size_t)finish_grid(c, count) * kBlock * kMaxQueues);
  auto next_event = [&]() {
    if (c->ev_used == c->ev_pool.size()) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreate(&e));
      c->ev_pool.push_back(e);
    }
    return c->ev_pool[c->ev_used++];
  };
  for (uint32_t done = 0; done < a->spp_count; done += spp_chunk) {
    uint32_t cs = std::min(spp_chunk, a->spp_count - done);
    const RenderParams rp = chunk_params(c, a, pl.first, n_pix, done, cs, (uint32_t)c->q[0].cap);
    if (a->max_depth == 0) continue;  // trace(ray, 0) returns (0, 0) for every sample: nothing to add
    // the queues, their shared work counter and the results slab
    uint32_t* work = c->work;
    float4* res = c->results;
    // fork: the queues start after the accumulate that last read the slab
    // (acc_done, on the caller's stream; the kernels read nothing else the
    // caller's stream writes)
    const uint32_t n0 = (uint32_t)std::min<size_t>(rp.G, c->pool_cap);
    HIP_CHECK(hipStreamWaitEvent(c->q[0].stream, c->acc_done, 0));
    HIP_CHECK(hipMemcpyAsync(work, &n0, 4, hipMemcpyHostToDevice, c->q[0].stream));
    HIP_CHECK(hipEventRecord(c->set_fork, c->q[0].stream));
    uint32_t base = 0;
    for (int k = 0; k < K; ++k) {
      Queue& q = c->q[k];
      const uint32_t nk = (uint32_t)(((uint64_t)n0 * (k + 1)) / K) - base;  // <= q.cap
      if (k) HIP_CHECK(hipStreamWaitEvent(q.stream, c->set_fork, 0));
      Ctrl init{{nk, 0}, 0, 0};
      HIP_CHECK(hipMemcpyAsync(q.ctrl, &init, sizeof(Ctrl), hipMemcpyHostToDevice, q.stream));
      if (nk) {
        hipLaunchKernelGGL(k_generate, dim3((nk + kBlock - 1) / kBlock), dim3(kBlock), 0, q.stream, c->cam, rp,
                           q.bufs[0], base, nk);
        HIP_CHECK(hipGetLastError());
      }
      base += nk;
    }
    std::vector<std::array<hipEvent_t, 3>> marks;
    std::vector<std::array<hipEvent_t, 2>> fin_marks;
    const int kBatch = 4;  // even: a status read sees the live pool in active[0]
    struct Loop {
      uint32_t it = 0;
      int slot = 0;
      bool pending = false, finished = false;
      size_t bound = ~(size_t)0;  // live paths at most (shade_grid)
      bool exhausted = false;     // the work counter was seen at or past G: no refill
    } st_[kMaxQueues];
    int open = K;
    // an internal error in the middle of a chunk: every queue's kernels end
    // before the error returns, so the next render does not fork onto pools
    // and a results slab that this chunk's launches still write
    auto fail_chunk = [&](const std::string& msg) {
      for (int k = 0; k < K; ++k) (void)hipStreamSynchronize(c->q[k].stream);
      throw ApiError{MRT_ERR_HIP, msg};
    };
    const ShadeFn shade = shade_kernel(count, c->scene_ext, c->tun.shade_wpe);
    while (open > 0) {
      for (int k = 0; k < K; ++k) {
        Queue& q = c->q[k];
        Loop& L = st_[k];
        if (L.finished) continue;
        for (int b = 0; b < kBatch; ++b, ++L.it) {
          const uint32_t cur = L.it & 1;
          std::array<hipEvent_t, 3> m{};
          if (timing) {
            m[0] = next_event();
            HIP_CHECK(hipEventRecord(m[0], q.stream));
          }
          if (simple)
            launch_trace_simple(c, q, cur);
          else
            launch_trace(c, q.stream, q, q.bufs[cur], cur, count, kTmin, INFINITY);
          if (timing) {
            m[1] = next_event();
            HIP_CHECK(hipEventRecord(m[1], q.stream));
          }
          hipLaunchKernelGGL(shade, dim3(shade_grid(q, L.bound)), dim3(kShadeBlock), 0, q.stream, c->S, rp, q.bufs[cur],
                             q.bufs[cur ^ 1], (const uint4*)q.hits, q.ctrl, cur, res, c->d_cnt);
          HIP_CHECK(hipGetLastError());
          if (!L.exhausted || rp.shade_bin == 2) {  // new paths behind the survivors (shade_bin 2: and the pool's ends joined)
            hipLaunchKernelGGL(k_reserve, dim3(1), dim3(64), 0, q.stream, q.ctrl, cur, work, rp.G, rp.pool_cap);
            hipLaunchKernelGGL(k_refill, dim3(c->refill_grid), dim3(kBlock), 0, q.stream, c->cam, rp, q.bufs[cur ^ 1],
                               (const Ctrl*)q.ctrl);
            HIP_CHECK(hipGetLastError());
          }
          if (timing) {
            m[2] = next_event();
            HIP_CHECK(hipEventRecord(m[2], q.stream));
            marks.push_back(m);
          }
        }
        hipLaunchKernelGGL(k_status, dim3(1), dim3(64), 0, q.stream, (const Ctrl*)q.ctrl, (const uint32_t*)work,
                           q.d_stat + L.slot);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(q.ev[L.slot], q.stream));
        if (L.pending) {  // the previous batch's status (one batch stays in flight)
          HIP_CHECK(hipEventSynchronize(q.ev[L.slot ^ 1]));
          const volatile HostStatus& v = q.h_stat[L.slot ^ 1];  // written by the GPU
          const HostStatus s{v.active0, v.active1, v.shade_short, v.work};
          if (s.shade_short)
            fail_chunk("internal: a k_shade grid was smaller than its live pool (" + std::to_string(s.shade_short) +
                       " paths)");
          if (s.work >= rp.G) {
            L.bound = std::min<size_t>(L.bound, s.active0);
            L.exhausted = true;
          }
          if (s.work >= rp.G && s.active0 <= finish_paths) {
            // no new work: the paths left (at most as many as that status
            // showed) finish in one fused launch after the batch just queued
            if (s.active0 > 0) {
              std::array<hipEvent_t, 2> fm{};
              if (timing) {
                fm[0] = next_event();
                HIP_CHECK(hipEventRecord(fm[0], q.stream));
              }
              launch_finish(c, k, L.it & 1, rp, count, res);
              if (timing) {
                fm[1] = next_event();
                HIP_CHECK(hipEventRecord(fm[1], q.stream));
                fin_marks.push_back(fm);
              }
            }
            L.finished = true;
            --open;
          }
        }
        L.pending = true;
        L.slot ^= 1;
        if (L.it > 64u * 1024u) fail_chunk("render did not converge");
      }
    }
    // join: `st` continues after every queue (which may still be running its
    // drain: the host does not wait)
    for (int k = 0; k < K; ++k) {
      HIP_CHECK(hipEventRecord(c->q[k].join, c->q[k].stream));
      HIP_CHECK(hipStreamWaitEvent(st, c->q[k].join, 0));
    }
    if (timing) {  // resolved by mrt_get_kernel_stats (resolve_kernel_timing)
      c->pend_marks.insert(c->pend_marks.end(), marks.begin(), marks.end());
      c->pend_fin.insert(c->pend_fin.end(), fin_marks.begin(), fin_marks.end());
    }
    hipLaunchKernelGGL(k_accumulate, dim3((n_pix + kAccPix - 1) / kAccPix), dim3(kBlock), 0, st, (const float4*)res,
                       n_pix, cs, (const uint32_t*)pl.first, d_rgb, d_b);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(c->acc_done, st));  // the slab is free again after this
  }
}

// Kernel timing of renders flagged MRT_RENDER_TIME_KERNELS, resolved when the
// stats are read (a timed render does not wait for its queue set's drain).
void resolve_kernel_timing(mrt_ctx* c) {
  if (c->pend_marks.empty() && c->pend_fin.empty()) return;
  for (auto& m : c->pend_marks) {
    float t0 = 0, t1 = 0;
    HIP_CHECK(hipEventSynchronize(m[2]));
    HIP_CHECK(hipEventElapsedTime(&t0, m[0], m[1]));
    HIP_CHECK(hipEventElapsedTime(&t1, m[1], m[2]));
    c->kstats.trace_ms += t0;
    c->kstats.shade_ms += t1;
    c->kstats.trace_launches++;
    c->kstats.shade_launches++;
    c->kstats.iterations++;
  }
  for (auto& m : c->pend_fin) {
    float t = 0;
    HIP_CHECK(hipEventSynchronize(m[1]));
    HIP_CHECK(hipEventElapsedTime(&t, m[0], m[1]));
    c->kstats.finish_ms += t;
    c->kstats.finish_launches++;
  }
  c->pend_marks.clear();
  c->pend_fin.clear();
  c->ev_used = 0;
}

extern "C" {

int mrt_render_device(mrt_ctx* c, const mrt_render_args* a, float* d_rgb, uint32_t* d_b, void* stream) {
  MRT_DEV0(c, mrt_render_device(c, a, d_rgb, d_b, stream));
  return guarded(c, [&] {
    if (!d_rgb || !d_b) throw ApiError{MRT_ERR_INVALID, "null accumulation buffer"};
    render_device(c, a, d_rgb, d_b, (hipStream_t)stream);  // NULL: the null stream
  });
}

int mrt_render(mrt_ctx* c, const mrt_render_args* a, float* rgb, uint32_t* bounces) {
  if (c && c->multi) return multi_render(c->multi, a, rgb, bounces, c->err);
  return guarded(c, [&] {
    if (!a || !rgb || !bounces) throw ApiError{MRT_ERR_INVALID, "null argument"};
    size_t np = (size_t)a->width * a->height;
    if (np > c->acc_cap) {
      hipFree(c->d_acc_rgb);
      hipFree(c->d_acc_b);
      c->d_acc_rgb = nullptr;
      c->d_acc_b = nullptr;
      HIP_CHECK(hipMalloc(&c->d_acc_rgb, np * 12));
      HIP_CHECK(hipMalloc(&c->d_acc_b, np * 4));
      c->acc_cap = np;
    }
    HIP_CHECK(hipMemcpyAsync(c->d_acc_rgb, rgb, np * 12, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(c->d_acc_b, bounces, np * 4, hipMemcpyHostToDevice, c->stream));
    render_device(c, a, c->d_acc_rgb, c->d_acc_b, c->stream);
    HIP_CHECK(hipMemcpyAsync(rgb, c->d_acc_rgb, np * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(bounces, c->d_acc_b, np * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
  });
}

}  // extern "C"
