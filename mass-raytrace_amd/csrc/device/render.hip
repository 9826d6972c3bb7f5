// render.hip — the wavefront path-tracing integrator for gfx950.
//
// Replaces render()'s per-thread pixel loop (main.rs:235-290): each sample
// (one camera path, main.rs:257-263) becomes a path slot in a pool of SoA
// HBM buffers, advanced one segment per iteration by two kernels:
//   k_trace : closest hit of every active ray (World::intersect; trace.hip) [k2]
//   k_shade : emit/scatter/background, path termination and wave
//             ballot/prefix-sum compaction of the survivors           [k3,k4]
//   k_reserve + k_refill<SRC> : new paths for the free slots behind the
//             survivors: camera rays (Camera::ray) or a caller's rays [k1]
// Finished samples are written to a per-(pixel,sample) result slab and folded
// into the caller's accumulation buffers in sample order by k_accumulate [k5]
// (Image::merge, main.rs:629-638), so the sums do not depend on scheduling
// or on how tiles are sharded across GPUs.
#include <algorithm>
#include <mutex>
#include <variant>

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

// Where a work item's camera comes from (CAM): the render's one camera, by
// value in the kernel's arguments, or a table of views (mrt_render_views); a
// table of rays (mrt_render_rays) has its own gen_work below.
// work_camera gives the camera and the stream seed of pixel-list entry p and
// leaves in p the pixel within its frame.
__device__ __forceinline__ const DevCamera& work_camera(const DevCamera& cam, const RenderParams& rp, uint32_t& p,
                                                        unsigned long long& seed) {
  seed = rp.seed;
  return cam;
}
// The entry is a global pixel P = v W H + p (loop.h view_split): view v's
// camera and seed, loaded per lane from the table (a few hundred bytes that
// every wave reads: cache hits), and p as view v's own render has it, so the
// path draws from the stream of that render.
__device__ __forceinline__ const DevCamera& work_camera(const ViewTable& t, const RenderParams& rp, uint32_t& p,
                                                        unsigned long long& seed) {
  const ViewPixel vp = view_split(p, t.pix_per_view);
  const DevView& w = t.views[MRT_IDX(t, vp.v, t.n_views, 26)];
  p = vp.p;
  seed = w.seed;
  return w.cam;
}

template <typename CAM>
__device__ __forceinline__ void gen_work(const CAM& cam, const RenderParams& rp, uint32_t g, float4& ro, float4& rd,
                                         uint4& rs) {
  // work items run sample-minor: the samples of one pixel are consecutive
  // (camera rays of a wave nearly equal), and the results slab is laid out
  // the same way, g = pixel * spp + sample
  uint32_t lp = g / rp.spp;
  uint32_t s_local = g - lp * rp.spp;
  uint32_t p = rp.pixlist[lp];  // lp < n_pix by construction (g < G)
  unsigned long long seed;
  const DevCamera& c = work_camera(cam, rp, p, seed);
  uint32_t y = p / rp.W, x = p - y * rp.W;
  PathRng rng = path_rng(seed, p, rp.sample_base + s_local);
  V3 o, d;
  camera_ray(c, x, y, rp.W, rp.H, rng, o, d);
  ro = make_float4(o.x, o.y, o.z, __uint_as_float(g));
  rd = make_float4(d.x, d.y, d.z, __uint_as_float(0u));
  rs = rng_pack(rng);
}

// A third source (mrt_render_rays): the path's start comes from a table of
// rays instead of a camera. Work item g is sample s of entry i (loop.h
// ray_work); the lane loads its 32-B entry as two quads (consecutive entries:
// a wave reads at most 2 KiB contiguous), takes the stream of (seed, key,
// sample) and advances it by the entry's skip, the draws whoever built the ray
// already took. The record is a camera path's: ro.w the work item, rd.w 0
// bounces. No pixel list is read: the result index is the list position.
__device__ __forceinline__ void gen_work(const RayTable& t, const RenderParams& rp, uint32_t g, float4& ro, float4& rd,
                                         uint4& rs) {
  const RayWork w = ray_work(g, rp.spp);
  const uint4* e = reinterpret_cast<const uint4*>(t.rays + MRT_IDX(t, w.i, t.n, 27));
  const uint4 a = e[0], b = e[1];  // {o.x, o.y, o.z, d.x} {d.y, d.z, key, skip}
  PathRng rng = path_rng(rp.seed, b.z, rp.sample_base + w.s);
  for (uint32_t k = ray_skip(b.w); k != 0; --k) rng.next();
  ro = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(g));
  rd = make_float4(__uint_as_float(a.w), __uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(0u));
  rs = rng_pack(rng);
}

// The new camera path of work item g into slot i of a pool.
template <typename CAM>
__device__ __forceinline__ void gen_path(const CAM& cam, const RenderParams& rp, const PathBufs& out, uint32_t g,
                                         uint32_t i) {
  float4 ro, rd;
  uint4 rs;
  gen_work(cam, rp, g, ro, rd, rs);
  out.ro[i] = ro;
  out.rd[i] = rd;
  out.thr[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);  // L = 0: rad not written
  out.rng[i] = rs;
}

// Initial pool: work items [base, base + n0) into slots [0, n0). SRC: where a
// path starts (DevCamera, ViewTable or RayTable; with_source chooses).
template <typename SRC>
__global__ __launch_bounds__(kBlock) void k_generate(SRC src, RenderParams rp, PathBufs out, uint32_t base,
                                                     uint32_t n0) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n0) return;
  gen_path(src, rp, out, base + i, i);
}

// The identity list of a ray list's render: k_accumulate adds list entry i's
// samples to accum[list[i]], and entry i of a ray list is its own result index.
__global__ __launch_bounds__(kBlock) void k_identity(uint32_t* list, uint32_t n) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) list[i] = i;
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
// What to generate and what to move is loop.h's plan_refill.
__global__ void k_reserve(Ctrl* ctrl, uint32_t cur, uint32_t* work, uint32_t G, uint32_t cap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long sv = ctrl->surv[cur ^ 1];  // 0 unless shade_bin 2
  const uint32_t lo = ctrl->active[cur ^ 1] + (uint32_t)sv, hi = (uint32_t)(sv >> 32);
  const uint32_t want = refill_want(lo + hi, cap);
  uint32_t base = G;
  if (want && __hip_atomic_load(work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < G) base = atomicAdd(work, want);
  const RefillPlan p = plan_refill(lo, hi, cap, G, base);
  ctrl->gen_slot = p.gen_slot;
  ctrl->gen_count = p.gen_count;
  ctrl->gen_base = p.gen_base;
  ctrl->gen_move = p.gen_move;
  ctrl->gen_move_src = p.gen_move_src;
  ctrl->gen_move_dst = p.gen_move_dst;
  ctrl->active[cur ^ 1] = p.active;
  ctrl->surv[cur ^ 1] = 0;
}

// ... and generate them (camera rays of consecutive work items, i.e. pixel
// order): the next k_trace finds the new paths together behind the
// survivors instead of scattered among them one per finished slot.
template <typename CAM>
__device__ __forceinline__ void refill(const CAM& cam, const RenderParams& rp, const PathBufs& out, const Ctrl* ctrl) {
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
  for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < m; j += gridDim.x * kBlock)
    gen_path(cam, rp, out, base + j, slot + j);
}
template <typename SRC>
__global__ __launch_bounds__(kBlock) void k_refill(SRC src, RenderParams rp, PathBufs out, const Ctrl* ctrl) {
  refill(src, rp, out, ctrl);
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
  // the live count (shade_workgroups), so a drain launch does not dispatch a
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

// Sizes a render's path pool and results slab to the device:
// they must fit the memory free now minus mem_reserve, since several
// contexts may share one device (a multi-device context over {0,0,0}, ranks
// rehearsed on one GPU) and the defaults alone ask for ~98 GiB. When either
// buffer has to grow both are released and planned afresh (loop.h's
// plan_sizes: the pool shrinks first, then the samples per results chunk).
// The planning of the contexts of a process is serialised, so each sees the
// others' buffers.
std::mutex g_alloc_mutex;
void plan_buffers(mrt_ctx* c, uint32_t n_pix, uint32_t& spp_chunk, bool need_pool) {
  std::lock_guard<std::mutex> lock(g_alloc_mutex);
  if (pool_wanted(n_pix, spp_chunk, c->tun.pool_paths, need_pool) <= c->pool_cap &&
      (size_t)n_pix * spp_chunk <= c->results.n)
    return;
  HIP_CHECK(hipDeviceSynchronize());  // the queues may still use the old buffers
  release_pool(c);
  HIP_CHECK(c->results.free());
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const size_t reserve = c->tun.mem_reserve;
  const size_t budget = free_b > reserve ? free_b - reserve : 0;
  const SizePlan plan = plan_sizes(n_pix, spp_chunk, c->tun.pool_paths, c->tun.queues, budget, need_pool);
  if (!plan.fits)
    throw ApiError{MRT_ERR_NOMEM, "device memory: " + std::to_string(free_b >> 20) + " MiB free, mem_reserve_mb " +
                                      std::to_string(reserve >> 20) + ": not even one sample per pixel fits"};
  spp_chunk = plan.spp_chunk;
  if (plan.P) ensure_pool(c, plan.P);
  HIP_CHECK(c->results.alloc((size_t)n_pix * spp_chunk));
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
  HIP_CHECK(hipMemsetAsync(&q.ctrl.p->next_work, 0, 4, q.stream));
  hipLaunchKernelGGL(render_kernel(count, c->scene_alpha, true), dim3(grid), dim3(kBlock), 0, q.stream, c->S, c->cam, rp,
                     sro, srd, q.ctrl.p, res, c->d_cnt.p, c->tun.trace, q.bufs[cur], cur);
  HIP_CHECK(hipGetLastError());
}

// The accumulation buffers a render adds to, on the device or (Staging) the
// caller's on the host. moments set: mrt_render_adaptive's, whose accumulate
// (adaptive.hip) adds the moments and counts beside the same sums.
struct Accum {
  float* rgb;
  uint32_t* bounces;
  float* moments = nullptr;
  uint32_t* samples = nullptr;
};

// Folds a chunk's results slab into the accumulation buffers on `st`
// (k_accumulate: in sample order).
void accumulate(mrt_ctx* c, const RenderParams& rp, const Accum& acc, hipStream_t st) {
  if (acc.moments) return accumulate_moments(c, rp, acc.rgb, acc.bounces, acc.moments, acc.samples, st);
  hipLaunchKernelGGL(k_accumulate, dim3((rp.n_pix + kAccPix - 1) / kAccPix), dim3(kBlock), 0, st,
                     (const float4*)c->results.p, rp.n_pix, rp.spp, rp.pixlist, acc.rgb, acc.bounces);
  HIP_CHECK(hipGetLastError());
}

// The fused path loop: one k_render launch + one k_accumulate per chunk.
void render_fused(mrt_ctx* c, const mrt_render_args* a, const uint32_t* pixlist_d, uint32_t n_pix, const Accum& acc,
                  hipStream_t st) {
  const bool count = (a->flags & MRT_RENDER_COUNTERS) != 0;
  const bool timing = (a->flags & MRT_RENDER_TIME_KERNELS) != 0;
  uint32_t spp_chunk = first_chunk(a->spp_count, c->tun.results_max, n_pix);
  plan_buffers(c, n_pix, spp_chunk, false);
  wait_queues(c, st);
  for (uint32_t done = 0; done < a->spp_count; done += spp_chunk) {
    const uint32_t cs = std::min(spp_chunk, a->spp_count - done);
    const RenderParams rp = chunk_params(c, a, pixlist_d, n_pix, done, cs, 0);
    const Ctrl init = ctrl_init(0);
    HIP_CHECK(hipMemcpyAsync(c->q[0].ctrl.p, &init, sizeof(Ctrl), hipMemcpyHostToDevice, st));
    if (timing) HIP_CHECK(hipEventRecord(c->tev[0], st));
    const RenderFn f = render_kernel(count, c->scene_alpha, false);
    const uint32_t grid = persistent_grid(c, (const void*)f, 0);
    ensure_slots(c, (size_t)grid * kBlock);
    hipLaunchKernelGGL(f, dim3(grid), dim3(kBlock), 0, st, c->S, c->cam, rp, c->slot_ro, c->slot_rd, c->q[0].ctrl.p,
                       c->results.p, c->d_cnt.p, c->tun.trace, PathBufs{}, 0u);
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
    accumulate(c, rp, acc, st);
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

void release_pool(mrt_ctx* c) {
  HIP_CHECK(c->pool.free());
  c->pool_cap = 0;
}

// P paths over the context's queues.
void ensure_pool(mrt_ctx* c, size_t P) {
  if (P <= c->pool_cap) return;
  HIP_CHECK(hipDeviceSynchronize());  // the queues may still be draining into the old pool
  release_pool(c);
  const int K = c->tun.queues;
  const size_t per_q = (P + K - 1) / K;
  HIP_CHECK(c->pool.alloc(pool_bytes(K, P)));
  char* p = c->pool.p;
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
  if (2 * n <= c->slots.n) return;
  if (c->slots.p) HIP_CHECK(hipDeviceSynchronize());  // a queue set's drain may still use them
  c->slot_ro = c->slot_rd = nullptr;
  HIP_CHECK(c->slots.alloc(2 * n));
  c->slot_ro = c->slots.p;
  c->slot_rd = c->slots.p + n;
}

// MRT_TILE x MRT_TILE tiles in raster order; shard si of sc owns t % sc == si;
// pixels of a tile in raster order, y = 0 the bottom row (main.rs:253-263)
std::vector<uint32_t> shard_pixel_list(uint32_t W, uint32_t H, uint32_t si, uint32_t sc) {
  return shard_list(W, H, si, sc, MRT_TILE);
}

// n_views == 0: the shard's list of one frame; else that list once per view
// as global pixels (loop.h view_list), for mrt_render_views.
std::pair<uint32_t*, uint32_t> pixlist(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc, uint32_t n_views) {
  auto key = std::make_tuple(W, H, si, sc, n_views);
  auto it = c->pixlists.find(key);
  if (it == c->pixlists.end()) {
    std::vector<uint32_t> list = shard_pixel_list(W, H, si, sc);
    if (n_views) list = view_list(list, n_views, W * H);
    DevBuf<uint32_t> d;
    HIP_CHECK(d.alloc(list.size()));
    if (d.p) HIP_CHECK(hipMemcpy(d.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
    it = c->pixlists.emplace(key, std::move(d)).first;
  }
  return {it->second.p, (uint32_t)it->second.n};
}

// Work enqueued on a caller's stream `st` that writes the context's shared
// buffers (q[0].ctrl, the results slab, the lane-ray slots): the next
// wavefront render forks its queues after acc_done, so recording it here
// orders that render after this work too.
void mark_ctx_busy(mrt_ctx* c, hipStream_t st) { HIP_CHECK(hipEventRecord(c->acc_done, st)); }

namespace {

// The kernel-timing marks of a render: stamp(stream) records an event of the
// context's pool on the stream and returns it when the render is timed, null
// otherwise. A chunk's marks wait here until its queues are joined (keep),
// then in the context until the stats are read (resolve_kernel_timing).
struct Stamps {
  mrt_ctx* c;
  bool timing;
  std::vector<std::array<hipEvent_t, 3>> marks;  // an iteration: before k_trace, before k_shade, after the refill
  std::vector<std::array<hipEvent_t, 2>> fin;    // around a hand-off launch
  hipEvent_t stamp(hipStream_t s) {
    if (!timing) return nullptr;
    if (c->ev_used == c->ev_pool.size()) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreate(&e));
      c->ev_pool.push_back(e);
    }
    hipEvent_t e = c->ev_pool[c->ev_used++];
    HIP_CHECK(hipEventRecord(e, s));
    return e;
  }
  void keep() {  // resolved by mrt_get_kernel_stats (resolve_kernel_timing)
    c->pend_marks.insert(c->pend_marks.end(), marks.begin(), marks.end());
    c->pend_fin.insert(c->pend_fin.end(), fin.begin(), fin.end());
    marks.clear();
    fin.clear();
  }
};

// Where the paths of a render start, exactly one of: the context's camera, a
// batch of views (the cameras from the table), a caller's ray list (no camera
// at all). A new source is a table struct, a gen_work overload and one
// alternative here.
using Source = std::variant<DevCamera, ViewTable, RayTable>;

// The one place a source becomes a template argument: f(src) with a copy of
// the alternative, so k_generate / k_refill <decltype(src)> follow from it.
template <typename F>
void with_source(const Source& s, F&& f) {
  std::visit(f, s);
}

// What the chunks of one wavefront render share.
struct Pass {
  bool count, simple;
  uint32_t finish_paths;  // drain hand-off threshold (0: never)
  ShadeFn shade;
  Source src;
};

// What every render needs, of a frame or of a ray list (with loop.h samples_fit).
void check_scene(const mrt_ctx* c) {
  if (!c->has_scene) throw ApiError{MRT_ERR_STATE, "no scene uploaded"};
}

// The argument and state errors of a render, before anything is enqueued.
// (A batch of views brings its own cameras: need_camera false.)
void check_render_args(const mrt_ctx* c, const mrt_render_args* a, bool need_camera = true) {
  if (!a) throw ApiError{MRT_ERR_INVALID, "null render args"};
  check_scene(c);
  if (need_camera && !c->has_camera) throw ApiError{MRT_ERR_STATE, "no camera set"};
  if (a->width == 0 || a->height == 0) throw ApiError{MRT_ERR_INVALID, "empty image"};
  if ((uint64_t)a->width * a->height >= (1ull << 32)) throw ApiError{MRT_ERR_INVALID, "image too large"};
  if (a->shard_index >= (a->shard_count ? a->shard_count : 1))
    throw ApiError{MRT_ERR_INVALID, "shard_index >= shard_count"};
  if (!samples_fit(a->spp_begin, a->spp_count)) throw ApiError{MRT_ERR_INVALID, "sample index overflow"};
}

// What the scene rules out for the render's flags.
void check_render_flags(const mrt_ctx* c, const mrt_render_args* a) {
  const bool simple = (a->flags & MRT_RENDER_SIMPLE_TRACE) != 0;
  if (simple && c->scene_ext)
    throw ApiError{MRT_ERR_INVALID, "MRT_RENDER_SIMPLE_TRACE does not support composite surfaces, CubeMap backgrounds or Eve materials"};
  if ((a->flags & MRT_RENDER_FUSED) && !simple) {
    if (c->facts.trav_rng)
      throw ApiError{MRT_ERR_INVALID, "MRT_RENDER_FUSED does not support scenes whose traversal draws (Volume, Mix alpha)"};
    if (c->scene_ext)
      throw ApiError{MRT_ERR_INVALID, "MRT_RENDER_FUSED does not support composite surfaces, CubeMap backgrounds or Eve materials"};
  }
}

// fork: the queues start after the accumulate that last read the slab
// (acc_done, on the caller's stream; the kernels read nothing else the
// caller's stream writes). The shared work counter starts behind the chunk's
// first n0 paths, which k_generate deals over the queues' pools.
void fork_queues(mrt_ctx* c, const RenderParams& rp, const Pass& p) {
  const int K = c->tun.queues;
  const uint32_t n0 = (uint32_t)std::min<size_t>(rp.G, c->pool_cap);
  HIP_CHECK(hipStreamWaitEvent(c->q[0].stream, c->acc_done, 0));
  HIP_CHECK(hipMemcpyAsync(c->work.p, &n0, 4, hipMemcpyHostToDevice, c->q[0].stream));
  HIP_CHECK(hipEventRecord(c->set_fork, c->q[0].stream));
  uint32_t base = 0;
  for (int k = 0; k < K; ++k) {
    Queue& q = c->q[k];
    const uint32_t nk = queue_share(n0, K, k);  // <= q.cap
    if (k) HIP_CHECK(hipStreamWaitEvent(q.stream, c->set_fork, 0));
    const Ctrl init = ctrl_init(nk);
    HIP_CHECK(hipMemcpyAsync(q.ctrl.p, &init, sizeof(Ctrl), hipMemcpyHostToDevice, q.stream));
    if (nk) {
      const dim3 grid((nk + kBlock - 1) / kBlock);
      with_source(p.src, [&](auto src) {
        hipLaunchKernelGGL(k_generate<decltype(src)>, grid, dim3(kBlock), 0, q.stream, src, rp, q.bufs[0], base, nk);
      });
      HIP_CHECK(hipGetLastError());
    }
    base += nk;
  }
}

// kBatch iterations of queue q — k_trace, k_shade and the refill — and the
// status read behind them (k_status into slot L.slot, then the slot's event).
void enqueue_batch(mrt_ctx* c, Queue& q, QueueLoop& L, const RenderParams& rp, const Pass& p, Stamps& t) {
  for (int b = 0; b < kBatch; ++b, ++L.it) {
    const uint32_t cur = L.it & 1;
    const hipEvent_t m0 = t.stamp(q.stream);
    if (p.simple)
      launch_trace_simple(c, q, cur);
    else
      launch_trace(c, q.stream, q, q.bufs[cur], cur, p.count, kTmin, INFINITY);
    const hipEvent_t m1 = t.stamp(q.stream);
    hipLaunchKernelGGL(p.shade, dim3(shade_workgroups(q.cap, L.bound, kShadeBlock)), dim3(kShadeBlock), 0, q.stream,
                       c->S, rp, q.bufs[cur], q.bufs[cur ^ 1], (const uint4*)q.hits, q.ctrl.p, cur, c->results.p, c->d_cnt.p);
    HIP_CHECK(hipGetLastError());
    if (!L.exhausted || rp.shade_bin == 2) {  // new paths behind the survivors (shade_bin 2: and the pool's ends joined)
      hipLaunchKernelGGL(k_reserve, dim3(1), dim3(64), 0, q.stream, q.ctrl.p, cur, c->work.p, rp.G, rp.pool_cap);
      with_source(p.src, [&](auto src) {
        hipLaunchKernelGGL(k_refill<decltype(src)>, dim3(c->refill_grid), dim3(kBlock), 0, q.stream, src, rp,
                           q.bufs[cur ^ 1], (const Ctrl*)q.ctrl.p);
      });
      HIP_CHECK(hipGetLastError());
    }
    const hipEvent_t m2 = t.stamp(q.stream);
    if (t.timing) t.marks.push_back({m0, m1, m2});
  }
  hipLaunchKernelGGL(k_status, dim3(1), dim3(64), 0, q.stream, (const Ctrl*)q.ctrl.p, (const uint32_t*)c->work.p,
                     q.d_stat + L.slot);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(q.ev[L.slot], q.stream));
}

// an internal error in the middle of a chunk: every queue's kernels end
// before the error returns, so the next render does not fork onto pools
// and a results slab that this chunk's launches still write
[[noreturn]] void fail_chunk(mrt_ctx* c, const std::string& msg) {
  for (int k = 0; k < c->tun.queues; ++k) (void)hipStreamSynchronize(c->q[k].stream);
  throw ApiError{MRT_ERR_HIP, msg};
}

// Waits for the status of the batch before the one just queued (one batch
// stays in flight) and acts on what on_status makes of it; true: queue k
// finished.
bool read_status(mrt_ctx* c, int k, QueueLoop& L, const RenderParams& rp, const Pass& p, Stamps& t) {
  Queue& q = c->q[k];
  HIP_CHECK(hipEventSynchronize(q.ev[L.slot ^ 1]));
  const volatile HostStatus& v = q.h_stat[L.slot ^ 1];  // written by the GPU
  const HostStatus s{v.active0, v.active1, v.shade_short, v.work};
  const LoopStep step = on_status(L, s, rp.G, p.finish_paths);
  if (step == LoopStep::kShadeShort)
    fail_chunk(c, "internal: a k_shade grid was smaller than its live pool (" + std::to_string(s.shade_short) + " paths)");
  if (step == LoopStep::kHandOff) {
    const hipEvent_t f0 = t.stamp(q.stream);
    launch_finish(c, k, L.it & 1, rp, p.count, c->results.p);
    const hipEvent_t f1 = t.stamp(q.stream);
    if (t.timing) t.fin.push_back({f0, f1});
  }
  return step != LoopStep::kGoOn;
}

// The host loop of a chunk: every open queue in turn enqueues a batch and
// reads the status of its batch before, until each has finished.
void run_queues(mrt_ctx* c, const RenderParams& rp, const Pass& p, Stamps& t) {
  const int K = c->tun.queues;
  QueueLoop loop[kMaxQueues];
  int open = K;
  while (open > 0) {
    for (int k = 0; k < K; ++k) {
      QueueLoop& L = loop[k];
      if (L.finished) continue;
      enqueue_batch(c, c->q[k], L, rp, p, t);
      if (L.pending && read_status(c, k, L, rp, p, t)) --open;
      L.pending = true;
      L.slot ^= 1;
      if (L.it > kMaxIterations) fail_chunk(c, "render did not converge");
    }
  }
}

// join: `st` continues after every queue (which may still be running its
// drain: the host does not wait)
void join_queues(mrt_ctx* c, hipStream_t st) {
  for (int k = 0; k < c->tun.queues; ++k) {
    HIP_CHECK(hipEventRecord(c->q[k].join, c->q[k].stream));
    HIP_CHECK(hipStreamWaitEvent(st, c->q[k].join, 0));
  }
}

// The wavefront loop over a pixel list, every step from plan_buffers on: what
// a render of the context's camera, a render of a batch of views (a
// ViewTable; the list then holds global pixels) and a render of a caller's
// ray list (a RayTable; the list is the identity, width and height are not
// read) share.
// The drain hand-off needs no camera under either table: launch_finish's
// kernel only adopts live paths (ADOPT: gen_work is not in it), so the
// context's camera, set or not, is passed and never read.
// `acc`: the accumulate that folds each chunk (plain, or with moments).
void render_wavefront(mrt_ctx* c, const mrt_render_args* a, const uint32_t* pixlist_d, uint32_t n_pix,
                      const Source& src, const Accum& acc, hipStream_t st) {
  const bool count = (a->flags & MRT_RENDER_COUNTERS) != 0;
  const bool simple = (a->flags & MRT_RENDER_SIMPLE_TRACE) != 0;
  uint32_t spp_chunk = first_chunk(a->spp_count, c->tun.results_max, n_pix);
  plan_buffers(c, n_pix, spp_chunk, true);
  Stamps stamps{c, (a->flags & MRT_RENDER_TIME_KERNELS) != 0};
  if (stamps.timing && c->pend_marks.size() + c->pend_fin.size() > kMaxPendingMarks) resolve_kernel_timing(c);
  // the drain hand-off (launch_finish): the fused kernel has no traversal
  // draws or composite surfaces; its lane-ray slots are allocated here, before
  // any queue runs (ensure_slots reallocates)
  const bool can_finish = !c->facts.trav_rng && !c->scene_ext && !simple;
  const Pass p{count, simple, can_finish ? c->tun.finish_paths : 0u, shade_kernel(count, c->scene_ext, c->tun.shade_wpe),
               src};
  if (p.finish_paths) ensure_slots(c, (size_t)finish_grid(c, count) * kBlock * kMaxQueues);
  for (uint32_t done = 0; done < a->spp_count; done += spp_chunk) {
    const uint32_t cs = std::min(spp_chunk, a->spp_count - done);
    const RenderParams rp = chunk_params(c, a, pixlist_d, n_pix, done, cs, (uint32_t)c->q[0].cap);
    fork_queues(c, rp, p);
    run_queues(c, rp, p, stamps);
    join_queues(c, st);
    stamps.keep();
    accumulate(c, rp, acc, st);
    HIP_CHECK(hipEventRecord(c->acc_done, st));  // the slab is free again after this
  }
}

// Every entry point below is a check_* that throws the call's argument and
// state errors and enqueues nothing on a stream (it does fetch the pixel list,
// which the first call for a frame size builds and uploads), and a run_* that
// does the work; the ABI's host form stages the caller's buffers between them.
// A check returns the list to work over: the shard's pixels as pixlist gives
// them, once per view for a batch; empty where the render has nothing to add.
using Work = std::pair<uint32_t*, uint32_t>;
Work frame_work(mrt_ctx* c, const mrt_render_args* a, uint32_t n_views = 0) {
  if (a->spp_count == 0) return Work{};  // no list is built for a render without samples
  return pixlist(c, a->width, a->height, a->shard_index, a->shard_count ? a->shard_count : 1, n_views);
}
Work or_nothing(const mrt_render_args* a, const Work& w) {
  return nothing_to_add(a->spp_count, a->max_depth, w.second) ? Work{} : w;
}

// mrt_render(_device). Kept as it was: without samples or pixels the flags are
// not looked at; with depth 0 (trace(ray, 0) returns (0, 0)) they are.
Work check_render(mrt_ctx* c, const mrt_render_args* a) {
  check_render_args(c, a);
  const Work w = frame_work(c, a);
  if (w.second) check_render_flags(c, a);
  return or_nothing(a, w);
}
void run_render(mrt_ctx* c, const mrt_render_args* a, const Work& w, const Accum& acc, hipStream_t st) {
  if ((a->flags & MRT_RENDER_FUSED) && !(a->flags & MRT_RENDER_SIMPLE_TRACE))
    render_fused(c, a, w.first, w.second, acc, st);
  else
    render_wavefront(c, a, w.first, w.second, c->cam, acc, st);
}

// mrt_render_views(_device): one wavefront render over the shard's pixels of
// every view (loop.h view_list), the cameras and seeds from a table on the
// device. The pool and the results slab are planned for all views at once, so
// a batch of small frames fills the pool as one large frame does, and drains
// once per chunk.
Work check_views(mrt_ctx* c, const mrt_render_args* a, const mrt_view* views, uint32_t n_views) {
  if (!views || n_views == 0) throw ApiError{MRT_ERR_INVALID, "mrt_render_views: no views"};
  check_render_args(c, a, false);
  if (!views_fit(n_views, a->width, a->height))
    throw ApiError{MRT_ERR_INVALID, "mrt_render_views: n_views * width * height must be below 2^32"};
  if (a->flags & MRT_RENDER_FUSED)
    throw ApiError{MRT_ERR_INVALID, "mrt_render_views: MRT_RENDER_FUSED renders one camera"};
  check_render_flags(c, a);
  return or_nothing(a, frame_work(c, a, n_views));
}
void run_views(mrt_ctx* c, const mrt_render_args* a, const Work& w, const mrt_view* views, uint32_t n_views,
               const Accum& acc, hipStream_t st) {
  // the caller's views are consumed here. The host copy stays with the
  // context: the upload below reads it when queue 0's stream gets there, and
  // by the next batch it has (that batch's host loop read the status of
  // kernels behind it)
  std::vector<DevView>& table = c->views_h;
  table.resize(n_views);
  for (uint32_t v = 0; v < n_views; ++v) table[v] = DevView{dev_camera(views[v].camera), 0u, views[v].seed};
  if (c->views.n < n_views) {
    if (c->views.p) HIP_CHECK(hipDeviceSynchronize());  // the last batch's kernels may still read the old table
    HIP_CHECK(c->views.alloc(n_views));
  }
  // the table is written on queue 0's stream behind the last render's
  // accumulate (acc_done: every queue's kernels, the old table's readers, end
  // before it), and every fork of this render follows on that stream
  HIP_CHECK(hipStreamWaitEvent(c->q[0].stream, c->acc_done, 0));
  HIP_CHECK(hipMemcpyAsync(c->views.p, table.data(), (size_t)n_views * sizeof(DevView), hipMemcpyHostToDevice,
                           c->q[0].stream));
  const ViewTable vt{c->views.p, a->width * a->height, n_views, c->dbg.p};
  render_wavefront(c, a, w.first, w.second, vt, acc, st);
}

// mrt_render_rays(_device). `host`: the table is in host memory and its skips
// can be read; a table on the device can only be looked at from outside.
// false: nothing to add.
bool check_rays(const mrt_ctx* c, const mrt_path_ray* rays, uint32_t n_rays, uint32_t spp_begin, uint32_t spp_count,
                uint32_t max_depth, uint32_t flags, const void* rgb, const void* bounces, bool host) {
  if (!rgb || !bounces) throw ApiError{MRT_ERR_INVALID, "null accumulation buffer"};
  if (!rays || n_rays == 0) throw ApiError{MRT_ERR_INVALID, "mrt_render_rays: no rays"};
  if (flags & (MRT_RENDER_FUSED | MRT_RENDER_SIMPLE_TRACE))
    throw ApiError{MRT_ERR_INVALID, "mrt_render_rays: MRT_RENDER_FUSED and MRT_RENDER_SIMPLE_TRACE render one camera"};
  if (!samples_fit(spp_begin, spp_count)) throw ApiError{MRT_ERR_INVALID, "sample index overflow"};
  if (host) {
    const uint32_t bad = first_bad_skip(rays, n_rays);
    if (bad < n_rays)
      throw ApiError{MRT_ERR_INVALID, "mrt_render_rays: entry " + std::to_string(bad) + " has skip " +
                                          std::to_string(rays[bad].skip) + ", above MRT_RAY_SKIP_MAX"};
  }
  check_scene(c);
  if (!host && ((uintptr_t)rays & 15u))
    throw ApiError{MRT_ERR_INVALID, "mrt_render_rays: the device table must be 16-byte aligned"};
  return !nothing_to_add(spp_count, max_depth, n_rays);
}

// One wavefront render over the work items of a ray list on the device
// (loop.h ray_work), every step a frame's from plan_buffers on. The queues'
// generation kernels read the table, which the caller's stream may have just
// written: queue 0's stream, on which every fork of this render follows,
// waits for `st` as it stands now.
void run_rays(mrt_ctx* c, const mrt_path_ray* d_rays, uint32_t n_rays, uint64_t seed, uint32_t spp_begin,
              uint32_t spp_count, uint32_t max_depth, uint32_t flags, const Accum& acc, hipStream_t st) {
  if (c->ray_ids.n < n_rays) {
    if (c->ray_ids.p) HIP_CHECK(hipDeviceSynchronize());  // an earlier render's accumulate may still read the old list
    HIP_CHECK(c->ray_ids.alloc(n_rays));
    hipLaunchKernelGGL(k_identity, dim3((n_rays + kBlock - 1) / kBlock), dim3(kBlock), 0, st, c->ray_ids.p, n_rays);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(c->ids_ready, st));
  }
  HIP_CHECK(hipStreamWaitEvent(st, c->ids_ready, 0));  // the list's one fill, whatever stream it ran on
  HIP_CHECK(hipEventRecord(c->rays_ready, st));
  HIP_CHECK(hipStreamWaitEvent(c->q[0].stream, c->rays_ready, 0));
  const mrt_render_args a{n_rays, 1u, spp_begin, spp_count, seed, max_depth, 0u, 1u, flags};
  render_wavefront(c, &a, c->ray_ids.p, n_rays, RayTable{d_rays, n_rays, c->dbg.p}, acc, st);
}

// mrt_render_adaptive(_device): a frame's checks and the rule's own (a is not
// null), then an empty report. The shard's tiles: none (an empty frame) where
// the render has nothing to add.
AdaptFrame check_adaptive(mrt_ctx* c, const mrt_render_args* a, const mrt_adaptive_params* prm,
                          mrt_adaptive_report* report) {
  if (const char* why = adapt_render_error(prm, a->spp_begin, a->spp_count, a->flags))
    throw ApiError{MRT_ERR_INVALID, why};
  check_render_args(c, a);  // before the frame's size is trusted
  check_render_flags(c, a);
  const AdaptFrame f = adaptive_frame(c, a->width, a->height, a->shard_index, a->shard_count ? a->shard_count : 1);
  if (report) *report = mrt_adaptive_report{};
  return nothing_to_add(a->spp_count, a->max_depth, f.n_tiles) ? AdaptFrame{} : f;
}

// The rounds of the adaptive rule around the wavefront loop (massrt.h states
// the rule, host/adaptive.h its arithmetic). Round r is one render_wavefront
// over the open tiles' pixel list with the round's sample base and the
// moment-carrying accumulate: plan_buffers, the queues and the drain are a
// frame's. Behind it on `st` the open tiles are evaluated (k_adaptive_tiles)
// and the survivors' pixels compacted into the next list (adaptive_compact),
// whose length the host waits for: one word per round. So the call returns
// when its last kernel has ended.
void run_adaptive(mrt_ctx* c, const mrt_render_args* a, const mrt_adaptive_params* prm, const AdaptFrame& f,
                  const Accum& acc, mrt_adaptive_report* report, hipStream_t st) {
  const auto pl = pixlist(c, a->width, a->height, a->shard_index, f.sc);
  const uint32_t cap = a->spp_count, n_shard = pl.second;
  adaptive_scratch(c, f.n_tiles, n_shard);
  HIP_CHECK(hipMemsetAsync(c->ad_open.p, 1, f.n_tiles, st));  // every tile starts in the running
  const float tau2 = adapt_tau2(prm->threshold);
  const uint32_t* list = pl.first;
  uint32_t n_pix = n_shard, done = 0, round = 0;
  uint64_t samples = 0;
  AdaptWord w{n_shard, f.n_tiles};
  for (;; ++round) {
    const uint32_t cnt = adapt_round_count(*prm, cap, round, done);
    if (cnt) {
      mrt_render_args ra = *a;
      ra.spp_begin = a->spp_begin + done;
      ra.spp_count = cnt;
      render_wavefront(c, &ra, list, n_pix, c->cam, acc, st);
      samples += (uint64_t)n_pix * cnt;
      done += cnt;
    }
    adaptive_evaluate(f, acc.moments, acc.samples, tau2, prm->floor, c->ad_open.p, true, nullptr, st);
    uint32_t* next = c->ad_list[round & 1].p;
    w = adaptive_compact(c, f, next, n_shard, round, st);
    list = next;
    n_pix = w.pixels;
    if (!adapt_goes_on(w.tiles, done, cap)) break;
  }
  mark_ctx_busy(c, st);
  if (report) *report = mrt_adaptive_report{round + 1, done, f.n_tiles, w.tiles, samples};
}

// The host forms' staging: the caller's accumulation buffers of n pixels or
// rays pass through the context's own on c->stream.
struct Staging {
  mrt_ctx* c;
  size_t n;
  Accum host;
  // one buffer, host to device (in) or back: its device pointer, null for one the caller does not have
  template <typename T>
  T* pass(DevBuf<T>& d, T* h, size_t count, bool in) {
    if (!h) return nullptr;
    if (in) HIP_CHECK(d.reserve(count));
    HIP_CHECK(in ? hipMemcpyAsync(d.p, h, count * sizeof(T), hipMemcpyHostToDevice, c->stream)
                 : hipMemcpyAsync(h, d.p, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return d.p;
  }
  Accum all(bool in) {
    return Accum{pass(c->d_acc_rgb, host.rgb, 3 * n, in), pass(c->d_acc_b, host.bounces, n, in),
                 pass(c->d_acc_mom, host.moments, 2 * n, in), pass(c->d_acc_n, host.samples, n, in)};
  }
  Accum in() { return all(true); }  // the buffers on the device
  void out() {
    all(false);
    HIP_CHECK(hipStreamSynchronize(c->stream));
  }
};

}  // namespace

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
    const Work w = check_render(c, a);
    if (w.second) run_render(c, a, w, {d_rgb, d_b}, (hipStream_t)stream);  // NULL: the null stream
  });
}

int mrt_render(mrt_ctx* c, const mrt_render_args* a, float* rgb, uint32_t* bounces) {
  if (c && c->multi) return multi_render(c->multi, a, rgb, bounces, c->err);
  return guarded(c, [&] {
    if (!a || !rgb || !bounces) throw ApiError{MRT_ERR_INVALID, "null argument"};
    const Work w = check_render(c, a);
    if (!w.second) return;  // nothing to add: the buffers stay as they are
    Staging s{c, (size_t)a->width * a->height, {rgb, bounces}};
    run_render(c, a, w, s.in(), c->stream);
    s.out();
  });
}

int mrt_render_views_device(mrt_ctx* c, const mrt_render_args* a, const mrt_view* views, uint32_t n_views,
                            float* d_rgb, uint32_t* d_b, void* stream) {
  MRT_DEV0(c, mrt_render_views_device(c, a, views, n_views, d_rgb, d_b, stream));
  return guarded(c, [&] {
    if (!d_rgb || !d_b) throw ApiError{MRT_ERR_INVALID, "null accumulation buffer"};
    const Work w = check_views(c, a, views, n_views);
    if (w.second) run_views(c, a, w, views, n_views, {d_rgb, d_b}, (hipStream_t)stream);  // NULL: the null stream
  });
}

int mrt_render_views(mrt_ctx* c, const mrt_render_args* a, const mrt_view* views, uint32_t n_views, float* rgb,
                     uint32_t* bounces) {
  MRT_DEV0(c, mrt_render_views(c, a, views, n_views, rgb, bounces));
  return guarded(c, [&] {
    if (!a || !rgb || !bounces) throw ApiError{MRT_ERR_INVALID, "null argument"};
    const Work w = check_views(c, a, views, n_views);
    if (!w.second) return;
    Staging s{c, (size_t)n_views * a->width * a->height, {rgb, bounces}};  // the views' frames, one behind the other
    run_views(c, a, w, views, n_views, s.in(), c->stream);
    s.out();
  });
}

int mrt_render_rays_device(mrt_ctx* c, const mrt_path_ray* d_rays, uint32_t n_rays, uint64_t seed, uint32_t spp_begin,
                           uint32_t spp_count, uint32_t max_depth, uint32_t flags, float* d_rgb, uint32_t* d_b,
                           void* stream) {
  MRT_DEV0(c, mrt_render_rays_device(c, d_rays, n_rays, seed, spp_begin, spp_count, max_depth, flags, d_rgb, d_b,
                                     stream));
  return guarded(c, [&] {
    if (check_rays(c, d_rays, n_rays, spp_begin, spp_count, max_depth, flags, d_rgb, d_b, false))
      run_rays(c, d_rays, n_rays, seed, spp_begin, spp_count, max_depth, flags, {d_rgb, d_b},
               (hipStream_t)stream);  // NULL: the null stream
  });
}

int mrt_render_adaptive_device(mrt_ctx* c, const mrt_render_args* a, const mrt_adaptive_params* params, float* d_rgb,
                               uint32_t* d_b, float* d_moments, uint32_t* d_samples, mrt_adaptive_report* report,
                               void* stream) {
  MRT_DEV0(c, mrt_render_adaptive_device(c, a, params, d_rgb, d_b, d_moments, d_samples, report, stream));
  return guarded(c, [&] {
    if (!a) throw ApiError{MRT_ERR_INVALID, "null render args"};
    if (!d_rgb || !d_b || !d_moments || !d_samples) throw ApiError{MRT_ERR_INVALID, "null accumulation buffer"};
    const AdaptFrame f = check_adaptive(c, a, params, report);
    if (f.n_tiles) run_adaptive(c, a, params, f, {d_rgb, d_b, d_moments, d_samples}, report, (hipStream_t)stream);
  });
}

int mrt_render_adaptive(mrt_ctx* c, const mrt_render_args* a, const mrt_adaptive_params* params, float* rgb,
                        uint32_t* bounces, float* moments, uint32_t* samples, mrt_adaptive_report* report) {
  MRT_DEV0(c, mrt_render_adaptive(c, a, params, rgb, bounces, moments, samples, report));
  return guarded(c, [&] {
    if (!a || !rgb || !bounces || !moments || !samples) throw ApiError{MRT_ERR_INVALID, "null argument"};
    const AdaptFrame f = check_adaptive(c, a, params, report);
    if (!f.n_tiles) return;
    Staging s{c, (size_t)a->width * a->height, {rgb, bounces, moments, samples}};
    run_adaptive(c, a, params, f, s.in(), report, c->stream);
    s.out();
  });
}

int mrt_render_rays(mrt_ctx* c, const mrt_path_ray* rays, uint32_t n_rays, uint64_t seed, uint32_t spp_begin,
                    uint32_t spp_count, uint32_t max_depth, uint32_t flags, float* rgb, uint32_t* bounces) {
  MRT_DEV0(c, mrt_render_rays(c, rays, n_rays, seed, spp_begin, spp_count, max_depth, flags, rgb, bounces));
  return guarded(c, [&] {
    if (!check_rays(c, rays, n_rays, spp_begin, spp_count, max_depth, flags, rgb, bounces, true)) return;
    // the table goes into the context's own buffer; the last host-form call's
    // kernels, its only readers, ended before that call returned
    HIP_CHECK(c->rays_d.reserve(n_rays));
    HIP_CHECK(hipMemcpyAsync(c->rays_d.p, rays, (size_t)n_rays * sizeof(mrt_path_ray), hipMemcpyHostToDevice,
                             c->stream));
    Staging s{c, n_rays, {rgb, bounces}};
    run_rays(c, c->rays_d.p, n_rays, seed, spp_begin, spp_count, max_depth, flags, s.in(), c->stream);
    s.out();
  });
}

}  // extern "C"
