// trace.hip — the closest hit of every active ray of a path pool
// (World::intersect): the persistent k_trace, the choice among its variants,
// its launch, and mrt_trace_rays, which sends arbitrary rays through it.
#include <string.h>

#include <algorithm>

#include "ctx.h"

using namespace mrt;

namespace {

// Persistent closest-hit kernel: a fixed grid of waves pulls chunks of rays
// from a counter; inside a wave a lane whose ray has finished takes the next
// ray of the wave's chunk as soon as enough lanes are idle, so the SIMD keeps
// issuing for busy lanes instead of waiting for the wave's slowest ray.
//
// LDS=true: the scene's treelet (layout.h, upload.cpp build_treelet) is first
// copied into the workgroup's LDS; records with an LDS-tagged index are then
// read there (ds_read_b128) instead of through L1/L2 — the top of the trees,
// which every ray visits, and small instanced BLAS whole. BLK threads per
// workgroup share one copy.
constexpr size_t kTraceLdsMaxBytes = 160 * 1024;
constexpr uint32_t kStashQuads = 4;  // float4s per lane of the world-ray stash (TravIn::stash)

// RNG: the scene's traversal draws random numbers (Volume, Mix alpha tests):
// each ray carries its path stream through the traversal and stores it back.
// (One ray per lane: two, interleaved for ILP, were measured slower at 84 VGPRs.)
// NF: the verified near-first walk (walk_nf.h trav_*_nf): the SAH trees walked
// near child first with a per-lane stack in LDS (kNfStack x BLK words of
// dynamic shared memory), the winner checked against the reference tree,
// rays that fail the check walked again the reference's way.
template <bool COUNT, bool LDS, uint32_t ALPHA, bool RNG, int BLK, bool NF = false, bool WILD = false, bool VBLAS = false>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(NF ? (COUNT ? 1 : 5) : (ALPHA == 0 && !RNG && !COUNT ? 8 : 1)))) void k_trace(DevScene S, PathBufs in, uint4* hits, Ctrl* ctrl, uint32_t cur,
                                                  DevCounters* cnt, float tmin, float tmax, TraceTune tune) {
  static_assert(!NF || (!LDS && !RNG), "the near-first walk has no treelet and no traversal draws");
  static_assert(!WILD || NF, "only the near-first walk has a wild tree");
  static_assert(!VBLAS || RNG, "a volume draws");
  const uint32_t n = ctrl->active[cur];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->active[cur ^ 1] = 0;
    ctrl->surv[cur ^ 1] = 0;
  }
  if (n == 0) return;  // uniform: every workgroup reads the same n
  if (LDS) {
    for (uint32_t k = threadIdx.x; k < S.n_tlet; k += BLK) mrt_lds[k] = reinterpret_cast<const uint4*>(S.tlet)[k];
    __syncthreads();
  }
  TravIn tin_{S, reinterpret_cast<const uint4*>(LDS ? S.slots_tl : S.slots), LDS ? S.tl_world_begin : S.world_begin,
              in.ro, in.rd, tmin, in.rng, tmax};
  if (!LDS && !NF) {  // the reference walk without a treelet: LDS holds the world-ray stash (TravIn::stash)
    tin_.stash = reinterpret_cast<float4*>(mrt_lds) + threadIdx.x;
    tin_.stash_stride = (uint32_t)BLK;
  }
  const TravIn& tin = tin_;
  const NfStack stk{reinterpret_cast<uint32_t*>(mrt_lds) + threadIdx.x, (uint32_t)BLK};
  LocalCounters lc;
  uint32_t seg = 0, nh = 0;
  uint32_t pool = 0, pool_end = 0;  // wave-uniform chunk [pool, pool_end)
  bool drained = false;             // wave-uniform: every group's share is taken
  // XCD-aware ray ranges: the pool is roughly in pixel order (camera rays in
  // tile order, survivors compacted in order), so giving each XCD group a
  // contiguous eighth keeps an XCD's rays — and the scene parts they touch —
  // together in that XCD's L2. A group whose eighth is taken helps the next.
  uint32_t grp = blockIdx.x % kGroups, visited = 0;  // wave-uniform
  Trav t{};  // fully initialised: idle lanes must not carry undefined state
  t.done = true;
  t.ray = kIdle;
  // The loop's phases, in order: refill, box run, mixed step / primitive run,
  // near-first batches, retire. They stay inline: as lambdas called from the
  // loop, the same statements made k_trace 1.7% slower on cube_field.
  for (;;) {
    // refill: once enough lanes are idle, the wave's next chunk starts on them
    const unsigned long long idle = __ballot(t.ray == kIdle);
    const uint32_t n_idle = (uint32_t)__popcll(idle);
    if (n_idle >= tune.refill || n_idle == 64u) {
      while (pool == pool_end && !drained) {  // grab the next chunk (wave-uniform)
        const uint32_t lo = (uint32_t)((uint64_t)n * grp / kGroups), hi = (uint32_t)((uint64_t)n * (grp + 1) / kGroups);
        uint32_t b = 0;
        if (lane_id() == 0) b = atomicAdd(&ctrl->group_next[grp * 32], tune.chunk);
        b = __shfl(b, 0, 64);
        if (b < hi - lo) {
          pool = lo + b;
          pool_end = hi - pool > tune.chunk ? pool + tune.chunk : hi;
        } else if (++visited == kGroups) {
          drained = true;
        } else {
          grp = (grp + 1) % kGroups;
        }
      }
      const uint32_t avail = pool_end - pool;
      if (t.ray == kIdle) {
        const uint32_t r = lane_rank(idle);
        if (r < avail) {
          if constexpr (NF)
            trav_init_nf<WILD>(tin, stk, t, MRT_IDX(S, pool + r, n, 20), tmax, S.nf_world);
          else
            trav_init<RNG, LDS>(tin, t, MRT_IDX(S, pool + r, n, 20), tmax);
        }
      }
      pool += n_idle < avail ? n_idle : avail;
      if (__ballot(t.ray != kIdle) == 0) break;  // chunk source exhausted
    }
    // box run: keep stepping boxes with little per-step overhead while at
    // least tune.box_min lanes are at one (lanes reaching a primitive wait)
    // Two steps per loop iteration: with one, the compiler carried the
    // record just loaded into the loop-header registers with 8 v_mov per
    // step; unrolled, the two steps alternate register sets and the copies
    // are gone (sphere_grid 671 -> 703, cube_field 254 -> 266, mesh_ply
    // 740 -> 749 Msamples/s, same box).
    auto box_step = [&]() {  // false: too few lanes at a box
      // a done lane holds an END record (or an idle lane's zeros), never a
      // box, so the record's flag alone decides (no done mask in the ballot)
      const bool run_box = trav_at_box(t);
      const unsigned long long bm = __builtin_amdgcn_ballot_w64(run_box);
      if ((uint32_t)__popcll(bm) < tune.box_min) return false;
      if (run_box) trav_box_index_either<COUNT, NF, WILD>(tin, stk, t, lc);
      // (a lane at a box is not done: of trav_may_fetch only the waiting is asked)
      if (run_box && (!NF || !nf_parked<WILD>(t))) trav_fetch<LDS>(tin, t);
      if (COUNT) {
        lc.wave_slots += lane_id() == 0 ? 64u : 0u;
        lc.lane_steps += run_box ? 1u : 0u;
      }
      return true;
    };
    while (box_step() && box_step()) {
    }
    // idle lanes hold a done Trav; a near-first lane whose walk is over
    // waits for the check below.
    // One step per busy lane (a box, or a primitive once enough lanes wait
    // at one or no lane is at a box), then ONE record fetch for every lane
    // that moved: the address unit costs per wave instruction, so the box
    // and primitive lanes share the load pair instead of issuing one each.
    // Primitive run (the box run's mirror): while at least tune.prim_run
    // lanes are at a primitive, they step alone (a leaf's primitives one
    // after another) instead of paying the box branch beside each step —
    // the same code with the box lanes masked off, so nothing is inlined
    // twice. Every pass steps a lane: while the run is on, tune.prim_run >=
    // tune.prim_batch (options.h derive_tuning), so its lanes have prim_go.
    for (;;) {
      const bool busy = trav_may_fetch<NF, WILD>(t);
      const bool at_box = busy && trav_at_box(t);
      const unsigned long long box_mask = __ballot(at_box);
      const unsigned long long prim_mask = __ballot(busy && !at_box);
      // (the near-first walk only: the reference walk's k_trace, compiled
      // with this loop, lost 14% — 971 -> 832 on sphere_grid at any
      // threshold, profiles/r6_primrun/ — so there it folds to one step)
      const bool prim_run = NF && (uint32_t)__popcll(prim_mask) >= tune.prim_run;  // wave-uniform
      const bool box_go = at_box && !prim_run;
      const bool prim_go = (__popcll(prim_mask) >= tune.prim_batch || box_mask == 0) && busy && !at_box;
      if (box_go) trav_box_index_either<COUNT, NF, WILD>(tin, stk, t, lc);
      if (prim_go) trav_prim_index_either<COUNT, ALPHA, RNG, LDS, VBLAS, NF, WILD>(tin, stk, t, lc);
      if ((box_go || prim_go) && trav_may_fetch<NF, WILD>(t)) trav_fetch<LDS>(tin, t);
      if (COUNT) {
        lc.wave_slots += lane_id() == 0 ? 64u : 0u;
        lc.lane_steps += (box_go || prim_go) ? 1u : 0u;
      }
      if (!prim_run) break;
    }
    // near-first walks that are over: check their hits (done, or the
    // reference's walk from the start) — batched: the check is a few
    // hundred wave instructions, so finished lanes wait (holding an END
    // record) until tune.nf_batch of them can share one pass, or until no
    // lane is walking any more
    if (NF) {
      // lanes that have walked everything but the wild instances' tree
      // (walk_nf.h kNfWait) enter it as a batch, for the same reason: a
      // wild leaf's box test, the entry and the exit are the walk's longest
      // steps, and a wave pays for each once per pass, however few lanes
      // take it. Entered one lane at a time, as each ray's stack ran out,
      // they cost sphere_grid 15% of k_trace's time for 12% fewer box
      // tests; batched at nf_batch, -2.5% (at half of it +1.8%, at a
      // quarter +7%: DESIGN.md §5).
      // this lane's batch (the lanes holding `mine`) goes once nf_batch of them
      // wait, or when none of the lanes `others()` is left to wait for
      auto batch_go = [&](bool mine, auto others) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
        return m != 0 && ((uint32_t)__popcll(m) >= tune.nf_batch || __builtin_amdgcn_ballot_w64(others()) == 0) && mine;
      };
      if (WILD && batch_go(t.sp == kNfWait, [&]() { return trav_may_fetch<NF, WILD>(t); })) {
        nf_resume_wild(tin, t);
        trav_fetch<LDS>(tin, t);
      }
      const bool over = t.sp == kNfDone;
      if (batch_go(over, [&]() { return !t.done && !over; })) {
        nf_finish<COUNT>(tin, t, lc);
        if (!t.done) trav_fetch<LDS>(tin, t);
      }
    }
    // retire: finished rays' hits out, their lanes idle
    if (t.ray != kIdle && t.done) {
      if (RNG) trav_store_rng(tin, t);
      const Hit h = trav_hit<LDS>(tin, t);
      hits[t.ray] = make_uint4(__float_as_uint(h.t), h.prim, h.container, 0u);
      seg += 1;
      nh += t.prim != kRefNone;
      t.ray = kIdle;
    }
  }
  if (COUNT) flush_counters(cnt, lc, seg, nh, 0, 0);
}

// Debug/bisection variant (MRT_RENDER_SIMPLE_TRACE): one ray per thread,
// the whole traversal in closest_hit.
template <bool RNG>
__global__ __launch_bounds__(kBlock) void k_trace_simple(DevScene S, PathBufs in, uint4* hits, Ctrl* ctrl,
                                                         uint32_t cur, DevCounters* cnt) {
  const uint32_t n = ctrl->active[cur];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->active[cur ^ 1] = 0;
    ctrl->surv[cur ^ 1] = 0;
  }
  LocalCounters lc;
  uint32_t seg = 0, nh = 0;
  const TravIn tin{S, reinterpret_cast<const uint4*>(S.slots), S.world_begin, in.ro, in.rd, kTmin, in.rng};
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    PathRng rng{0, 0};
    if (RNG) rng = rng_unpack(in.rng[i]);
    Hit h = closest_hit<true, RNG>(tin, i, INFINITY, lc, rng);
    if (RNG) in.rng[i] = rng_pack(rng);
    hits[i] = make_uint4(__float_as_uint(h.t), h.prim, h.container, 0u);
    seg += 1;
    nh += h.prim != kRefNone;
  }
  flush_counters(cnt, lc, seg, nh, 0, 0);
}

// mrt_trace_rays: arbitrary rays go through the product k_trace. In: rays
// (6 floats each) -> pool slots; out: hit records -> mrt_hit with front_face.
__global__ __launch_bounds__(kBlock) void k_rays_in(const float* rays, uint32_t n, PathBufs out) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float* r = rays + 6 * (size_t)i;
  out.ro[i] = make_float4(r[0], r[1], r[2], __uint_as_float(i));
  out.rd[i] = make_float4(r[3], r[4], r[5], __uint_as_float(0u));
  out.rng[i] = rng_pack(path_rng(0, i, 0xFFFFFFFEu));  // traversal draws of mrt_trace_rays (massrt.h)
}

template <bool EXT>
__global__ __launch_bounds__(kBlock) void k_rays_out(DevScene S, PathBufs in, const uint4* hits, uint32_t n,
                                                     uint4* out) {
  uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 o4 = in.ro[i], d4 = in.rd[i];
  const uint4 hv = hits[i];
  Hit h{__uint_as_float(hv.x), hv.y, hv.z};
  uint32_t front = 0;
  LocalCounters lc;  // a mapped normal decides front_face (EXT): its taps are not counted
  if (h.prim != kRefNone)
    front = resolve_hit<EXT>(S, V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, h, lc).front_face ? 1u : 0u;
  // a NaN t (the reference's range checks are false on it: a hit): the bits
  // the oracle's host computes, which the device's own instructions need not
  // give (isect.h host_nan) — the winner's expression again by the host's rules
  if (h.prim != kRefNone && h.t != h.t) {
    V3 o{o4.x, o4.y, o4.z}, d{d4.x, d4.y, d4.z};
    const uint32_t pkind = h.prim >> 28, pidx = h.prim & 0x0FFFFFFFu;
    if (pkind == MRT_REF_SPHERE) {  // spheres are world objects
      const uint32_t sp = MRT_IDX(S, pidx, S.n_sph, 10);
      h.t = sphere_root_nan(ld3(S.sph + (size_t)sp * 4), S.sph[(size_t)sp * 4 + 3], o, d);
    } else if (pkind == MRT_REF_TRIANGLE) {
      if ((h.container >> 28) == MRT_REF_INSTANCE) {
        V3 c0, c1, c2, c3;
        load_m12(S.inst_inv + (size_t)MRT_IDX(S, h.container & 0x0FFFFFFFu, S.n_inst, 9) * 12, c0, c1, c2, c3);
        const V3 wo = o, wd = d;
        o = xform_nan(c0, c1, c2, c3, wo, 1.0f);
        d = xform_nan(c0, c1, c2, c3, wd, 0.0f);
      }
      const TriShade tr = load_tri(S, pidx);
      h.t = tri_t_nan(tr.a, tr.b - tr.a, tr.c - tr.a, o, d);
    }
  }
  out[i] = make_uint4(h.prim, h.container, __float_as_uint(h.prim != kRefNone ? h.t : 0.0f), front);
}

// The k_trace variant for a scene: counting or not; the record stream's top
// in LDS (a treelet, with the workgroup size that shares it); alpha tests
// none / plain surfaces / composite surfaces (EXT); traversal draws; or the
// near-first walk (scenes with NF trees, no treelet, no traversal draws).
using TraceFn = void (*)(DevScene, PathBufs, uint4*, Ctrl*, uint32_t, DevCounters*, float, float, TraceTune);
// rng: the traversal draws; vblas: and some volume's target is a BLAS (the
// nested searches of walk.h volume_hit_blas cost registers, so scenes without
// such a volume keep the kernels they had). A workgroup larger than kBlock
// exists only to share a treelet.
TraceFn trace_kernel(bool count, bool lds, uint32_t alpha, bool rng, bool vblas, int block, bool nf, bool wild) {
  return with_value<true, false>(count, [&](auto COUNT) {
    return with_value<2u, 1u, 0u>(alpha, [&](auto ALPHA) -> TraceFn {
      if (nf)
        return with_value<true, false>(wild, [&](auto WILD) -> TraceFn { return k_trace<COUNT, false, ALPHA, false, kBlock, true, WILD>; });
      return with_value<true, false>(rng, [&](auto RNG) {
        return with_value<true, false>(vblas, [&](auto VB) {
          return with_value<true, false>(lds, [&](auto LDS) {
            return with_value<1024, 512, kBlock>(block, [&](auto B) -> TraceFn {
              return k_trace<COUNT, LDS, ALPHA, RNG, LDS ? B : kBlock, false, false, RNG && VB>;  // a volume draws
            });
          });
        });
      });
    });
  });
}

}  // namespace

// Occupancy-sized persistent grid for kernel f with `smem` dynamic LDS.
// `shared`: the kernel runs beside the other queues' kernels (k_trace with
// several queues) — it takes 3/4 of the occupancy, so another queue's trace
// and shade launches find room on every CU instead of queueing behind a
// grid that holds the whole GPU until its last ray (sphere_grid, 2 queues:
// 8 WGs/CU 585, 6 WGs/CU 618 Msamples/s).
uint32_t persistent_grid(mrt_ctx* c, const void* f, size_t smem, bool shared, int block, int share_num,
                         int share_den) {
  auto key = std::make_pair(f, smem);
  auto it = c->grids.find(key);
  if (it != c->grids.end()) return it->second;
  if (smem > 0) HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTraceLdsMaxBytes));
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, block, smem));
  if (shared) per_cu = std::max(1, per_cu * share_num / share_den);
  if (c->tun.wgs_per_cu) per_cu = (int)c->tun.wgs_per_cu;
  const uint32_t g = (uint32_t)c->cus * (uint32_t)std::max(1, per_cu);
  c->grids[key] = g;
  return g;
}

void launch_trace(mrt_ctx* c, hipStream_t st, const Queue& q, const PathBufs& in, uint32_t cur, bool count,
                  float tmin, float tmax) {
  const Tuning& t = c->tun;
  const bool shared = t.queues > 1;  // beside the other queues' kernels (persistent_grid)
  const uint32_t alpha = c->scene_alpha ? (c->scene_ext ? 2u : 1u) : 0u;
  const bool rng = c->facts.trav_rng, vblas = rng && c->scene_vblas;
  // a scene with a wild tree (layout.h nf_wild_root) runs the variant that walks it last, in batches; the
  // others compile none of that and keep 24 stack words (the builder leaves them the marker's word unused)
  const bool nf = t.use_nf, wild = nf && c->S.nf_wild_root != 0;
  const bool lds = !nf && c->facts.treelet;
  const int block = lds ? t.trace_block : kBlock;
  const TraceFn f = trace_kernel(count, lds, alpha, rng, vblas, block, nf, wild);
  size_t smem;  // dynamic LDS
  uint32_t grid;
  if (nf) {
    // Near-first: 24 KiB of LDS per workgroup of 256 lanes, kNfStack (25) with a
    // wild tree, allow 6 workgroups per CU (6 x 25 = 150 of 160 KiB), i.e. 6
    // waves per SIMD, its
    // registers (<= 128 VGPRs: the rounding margins' state and code, round 5,
    // would spill at 80) at least 4. Beside another queue the walk takes 3
    // WG/CU: its vector-memory unit is the shared limit, so more of its waves
    // buy nothing while k_shade beside it gains (profiles/r4_nf/tune.txt §6:
    // 4 -> 3 WG/CU +0.8%, 2 WG/CU -14%)
    smem = (size_t)(kNfStack - (wild ? 0u : 1u)) * block * 4;  // the stack's words per lane
    grid = persistent_grid(c, (const void*)f, smem, shared, block, 1, 1);
    const uint32_t nf_cap = 3u * (uint32_t)c->cus;
    if (shared && !t.wgs_per_cu && grid > nf_cap) grid = c->grids[std::make_pair((const void*)f, smem)] = nf_cap;
  } else {
    smem = lds ? (size_t)c->S.n_tlet * 16 : (size_t)kStashQuads * block * 16;  // the treelet, or the world-ray stash (4 x 16 B per lane)
    grid = persistent_grid(c, (const void*)f, smem, shared, block, 3, 4);
  }
  hipLaunchKernelGGL(f, dim3(grid), dim3(block), smem, st, c->S, in, q.hits, q.ctrl.p, cur, c->d_cnt.p, tmin, tmax, t.trace);
  HIP_CHECK(hipGetLastError());
}

void launch_trace_simple(mrt_ctx* c, const Queue& q, uint32_t cur) {
  auto* f = c->facts.trav_rng ? k_trace_simple<true> : k_trace_simple<false>;
  hipLaunchKernelGGL(f, dim3(c->trace_grid), dim3(kBlock), 0, q.stream, c->S, q.bufs[cur], q.hits, q.ctrl.p, cur, c->d_cnt.p);
  HIP_CHECK(hipGetLastError());
}

extern "C" int mrt_trace_rays(mrt_ctx* c, const float* rays, uint32_t n, float t_min, float t_max, mrt_hit* out) {
  MRT_DEV0(c, mrt_trace_rays(c, rays, n, t_min, t_max, out));
  return guarded(c, [&] {
    if (!c->has_scene) throw ApiError{MRT_ERR_STATE, "no scene uploaded"};
    if (n == 0) return;
    if (!rays || !out) throw ApiError{MRT_ERR_INVALID, "null argument"};
    HIP_CHECK(c->d_rays.reserve((size_t)n * 6));
    HIP_CHECK(c->d_rhits.reserve(n));
    HIP_CHECK(hipMemcpyAsync(c->d_rays.p, rays, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
    wait_queues(c, c->stream);
    ensure_pool(c, (size_t)n * c->tun.queues);  // all rays go to queue 0
    const Queue& q = c->q[0];
    const uint32_t g = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_rays_in, dim3(g), dim3(kBlock), 0, c->stream, (const float*)c->d_rays.p, n, q.bufs[0]);
    HIP_CHECK(hipGetLastError());
    const Ctrl init = ctrl_init(n, /*next_work*/ n);
    HIP_CHECK(hipMemcpyAsync(q.ctrl.p, &init, sizeof(Ctrl), hipMemcpyHostToDevice, c->stream));
    launch_trace(c, c->stream, q, q.bufs[0], 0u, true, t_min, t_max);
    hipLaunchKernelGGL(c->scene_ext ? k_rays_out<true> : k_rays_out<false>, dim3(g), dim3(kBlock), 0, c->stream, c->S,
                       q.bufs[0], (const uint4*)q.hits, n, c->d_rhits.p);
    HIP_CHECK(hipGetLastError());
    std::vector<uint4> h(n);
    HIP_CHECK(hipMemcpyAsync(h.data(), c->d_rhits.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < n; ++i) {
      out[i].prim = h[i].x;
      out[i].container = h[i].y;
      memcpy(&out[i].t, &h[i].z, 4);
      out[i].front_face = h[i].w;
    }
  });
}
