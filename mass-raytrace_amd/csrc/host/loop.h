// loop.h — the integer decisions of the wavefront loop (render.hip): the
// refill and gap-closing plan of k_reserve, the sizes of the path pool and
// the results slab, the pixel lists of a shard and of a batch of views, the
// work items and limits of a caller's ray list, the split of a chunk's first
// paths over the queues, and what a queue does with a lagged status read.
// Plain C++, no HIP: every function here runs on the host in
// tools/loop_check.cpp (tests/test_loop.py), tools/views_check.cpp
// (tests/test_views.py) or tools/rays_check.cpp (tests/test_rays.py); those a
// kernel also calls carry MRT_HD.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../mrt_math.h"

// Lagged status read of a queue (k_status): the fields the host loop needs.
// (At global scope beside pool.h's Ctrl: k_status takes both.)
struct HostStatus {
  uint32_t active0, active1, shade_short, work;
};

namespace mrt {

// ---- refill (k_reserve -> k_refill) ----------------------------------------

// Work items a pool of `cap` slots with `n` survivors asks the work counter for.
MRT_HD uint32_t refill_want(uint32_t n, uint32_t cap) { return n < cap ? cap - n : 0u; }

// What k_reserve stores into Ctrl after its atomic: work items
// [gen_base, gen_base + gen_count) go to slots [gen_slot, gen_slot +
// gen_count) behind the survivors, gen_move paths go from gen_move_src.. to
// gen_move_dst.., and the pool then holds `active` paths in [0, active).
struct RefillPlan {
  uint32_t gen_slot, gen_count, gen_base, gen_move, gen_move_src, gen_move_dst, active;
};

// The refill of a pool of `cap` slots whose survivors sit in [0, lo) and
// (shade_bin 2) in [cap - hi, cap); `base` is what the work counter's
// atomicAdd(refill_want) returned, or G when none was issued (nothing wanted,
// or the counter already at or past G).
MRT_HD RefillPlan plan_refill(uint32_t lo, uint32_t hi, uint32_t cap, uint32_t G, uint32_t base) {
  const uint32_t n = lo + hi, want = refill_want(n, cap);
  const uint32_t m = base < G ? (G - base < want ? G - base : want) : 0u;
  // the top block [cap - hi, cap) closes onto the refill's end lo + m: its
  // paths at or past the new end E move into the free slots below E
  const uint32_t E = n + m, g = cap - E;
  const uint32_t mv = g < hi ? g : hi;
  // sources [cap - mv, cap) and destinations [lo + m, lo + m + mv) are
  // disjoint, and the pool stays contiguous: [0, E) live, nothing past it
  return RefillPlan{lo, m, base, mv, cap - mv, lo + m, E};
}

// ---- buffer sizes (plan_buffers) -------------------------------------------

// device bytes of a pool of P paths over `queues` queues: two state
// sets (5 x 16 B each) + the hit record per path, 256-B aligned sections
constexpr size_t kPathBytes = 16 * (2 * 5 + 1);
inline size_t pool_bytes(int queues, size_t P) {
  const size_t K = (size_t)queues, per_q = (P + K - 1) / K;
  return (kPathBytes * per_q + 4096) * K;
}

// the pool does not shrink below this many paths before the chunks do
constexpr size_t kPoolFloor = (size_t)64 << 20;

// The first samples per chunk of a render: results slab <= results_max
// samples (16 B each).
inline uint32_t first_chunk(uint32_t spp_count, uint64_t results_max, uint32_t n_pix) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(spp_count, results_max / n_pix));
}

// The pool a chunk of spp_chunk samples per pixel asks for: pool <= pool_paths.
inline size_t pool_wanted(uint32_t n_pix, uint32_t spp_chunk, size_t pool_paths, bool need_pool) {
  return need_pool ? std::min<size_t>((size_t)n_pix * spp_chunk, pool_paths) : 0;
}

// The pool (P paths) and the samples per results chunk that fit `budget`
// bytes: the pool shrinks first (its size barely matters from 128M paths on,
// DESIGN.md §4), down to kPoolFloor paths, then the samples per results chunk
// (more chunks, the same image: chunks accumulate in sample order). !fits:
// not even one sample per pixel fits.
struct SizePlan {
  size_t P;
  uint32_t spp_chunk;
  bool fits;
};
inline SizePlan plan_sizes(uint32_t n_pix, uint32_t spp_chunk, size_t pool_paths, int queues, size_t budget,
                           bool need_pool) {
  size_t P = pool_wanted(n_pix, spp_chunk, pool_paths, need_pool);
  for (;;) {
    const size_t need = (P ? pool_bytes(queues, P) : 0) + (size_t)n_pix * spp_chunk * 16;
    if (need <= budget) return SizePlan{P, spp_chunk, true};
    if (P > kPoolFloor) {
      P = std::max(kPoolFloor, P / 2);
    } else if (spp_chunk > 1) {
      spp_chunk = spp_chunk / 2;
      if (P) P = std::min<size_t>(P, (size_t)n_pix * spp_chunk);
    } else {
      return SizePlan{P, spp_chunk, false};
    }
  }
}

// ---- pixel lists (pixlist) --------------------------------------------------

// A shard's pixels p = y W + x: tile x tile tiles in raster order, shard si of
// sc owns the tiles t with t % sc == si; the pixels of a tile in raster order,
// y = 0 the bottom row (main.rs:253-263).
inline std::vector<uint32_t> shard_list(uint32_t W, uint32_t H, uint32_t si, uint32_t sc, uint32_t tile) {
  const uint32_t tx = (W + tile - 1) / tile, ty = (H + tile - 1) / tile;
  std::vector<uint32_t> list;
  for (uint32_t t = si; t < tx * ty; t += sc) {
    const uint32_t bx = (t % tx) * tile, by = (t / tx) * tile;
    for (uint32_t py = 0; py < tile; ++py)
      for (uint32_t px = 0; px < tile; ++px) {
        const uint32_t x = bx + px, y = by + py;
        if (x < W && y < H) list.push_back(y * W + x);
      }
  }
  return list;
}

// A render of n_views views of W x H pixels (mrt_render_views) runs over
// global pixels P = v W H + p: pixel p of view v, and at once the pixel's
// place in the caller's buffers, view v's frame behind view v - 1's. They fit
// 32 bits: n_views W H < 2^32.
inline bool views_fit(uint64_t n_views, uint32_t W, uint32_t H) {
  const uint64_t ppv = (uint64_t)W * H;  // < 2^64: no product below overflows
  return n_views > 0 && ppv > 0 && ppv < (1ull << 32) && n_views < (1ull << 32) && n_views * ppv < (1ull << 32);
}
MRT_HD uint32_t view_pixel(uint32_t v, uint32_t p, uint32_t pix_per_view) { return v * pix_per_view + p; }
struct ViewPixel {
  uint32_t v, p;
};
MRT_HD ViewPixel view_split(uint32_t P, uint32_t pix_per_view) {
  const uint32_t v = P / pix_per_view;
  return ViewPixel{v, P - v * pix_per_view};
}

// The pixel list of such a render: the shard's list once per view, view 0's
// first. Work items g = lp spp + s over it keep a view's samples together,
// so all but one wave per view boundary generate for a single view.
inline std::vector<uint32_t> view_list(const std::vector<uint32_t>& shard, uint32_t n_views, uint32_t pix_per_view) {
  std::vector<uint32_t> list;
  list.reserve(shard.size() * n_views);
  for (uint32_t v = 0; v < n_views; ++v)
    for (uint32_t p : shard) list.push_back(view_pixel(v, p, pix_per_view));
  return list;
}

// ---- ray lists (mrt_render_rays) --------------------------------------------

// A render of a caller's ray list runs over work items g = i spp + s: sample s
// of the chunk for entry i, sample-minor as a frame's (g = pixel spp + sample),
// so the results slab and k_accumulate see entry i where they see list pixel
// i, and the list k_accumulate takes is the identity.
struct RayWork {
  uint32_t i, s;
};
MRT_HD RayWork ray_work(uint32_t g, uint32_t spp) {
  const uint32_t i = g / spp;
  return RayWork{i, g - i * spp};
}

// Draws an entry's stream is advanced by before its path starts: its skip,
// at most kRaySkipMax (MRT_RAY_SKIP_MAX; the host form refuses more, the
// device form cannot look and clamps).
constexpr uint32_t kRaySkipMax = 4096u;
MRT_HD uint32_t ray_skip(uint32_t skip) { return skip < kRaySkipMax ? skip : kRaySkipMax; }

// The first entry of a host table whose skip is above the limit; n: none.
template <typename RAY>
inline uint32_t first_bad_skip(const RAY* rays, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i)
    if (rays[i].skip > kRaySkipMax) return i;
  return n;
}

// Samples [spp_begin, spp_begin + spp_count): the end fits 32 bits, the limit
// a frame's render has.
inline bool samples_fit(uint32_t spp_begin, uint32_t spp_count) {
  return (uint64_t)spp_begin + spp_count <= 0xFFFFFFFFull;
}

// A render of spp_count samples of depth max_depth over a list of n pixels or
// rays has nothing to add when any of the three is 0 (trace(ray, 0) returns
// (0, 0) for every sample): the buffers stay as they are, and nothing is
// planned or enqueued for it.
inline bool nothing_to_add(uint32_t spp_count, uint32_t max_depth, uint32_t n) {
  return spp_count == 0 || max_depth == 0 || n == 0;
}

// ---- the fork ---------------------------------------------------------------

// Queue k's share of a chunk's first n0 paths over K queues (<= ceil(P / K),
// the queue's capacity, for n0 <= the pool's P); the shares before it sum to
// its first work item.
inline uint32_t queue_share(uint32_t n0, int K, int k) {
  return (uint32_t)(((uint64_t)n0 * (k + 1)) / K) - (uint32_t)(((uint64_t)n0 * k) / K);
}

// ---- the per-queue loop -----------------------------------------------------

// k_shade's grid for a pool of `cap` slots known to hold at most `bound`
// live paths: one workgroup per `block` of them.
// While the work counter has items left the pool refills to capacity; once
// it is exhausted the live count only falls, so the last status the host
// read bounds every later launch — a drain launch then dispatches a few
// workgroups instead of one per 256 slots of the whole pool.
inline uint32_t shade_workgroups(size_t cap, size_t bound, uint32_t block) {
  const size_t n = std::min(cap, bound);
  return (uint32_t)std::max<size_t>(1, (n + block - 1) / block);
}

// Iterations (k_trace + k_shade + refill) a queue enqueues between two status
// reads. Even: a status read sees the live pool in active[0].
constexpr int kBatch = 4;
static_assert(kBatch % 2 == 0, "on_status reads the live pool from active0");

// A queue that ran this many iterations did not converge.
constexpr uint32_t kMaxIterations = 64u * 1024u;

// One queue's state in the host loop.
struct QueueLoop {
  uint32_t it = 0;
  int slot = 0;
  bool pending = false, finished = false;
  size_t bound = ~(size_t)0;  // live paths at most (shade_workgroups)
  bool exhausted = false;     // the work counter was seen at or past G: no refill
};

// What a queue does after a status read.
enum class LoopStep {
  kGoOn,        // enqueue the next batch
  kHandOff,     // finished: the paths left go to one fused launch (launch_finish)
  kFinished,    // finished: no path left (or no hand-off and none left)
  kShadeShort,  // fail: a k_shade grid was smaller than its live pool
};

// The status `s` of the batch before the one just queued, for a chunk of G
// work items: once the counter is exhausted the status bounds the live count
// (shade_workgroups) and the refill stops; then, with at most finish_paths
// paths left, the queue finishes — no new work: the paths left (at most as
// many as that status showed) finish in one fused launch after the batch
// just queued.
inline LoopStep on_status(QueueLoop& L, const HostStatus& s, uint32_t G, uint32_t finish_paths) {
  if (s.shade_short) return LoopStep::kShadeShort;
  if (s.work >= G) {
    L.bound = std::min<size_t>(L.bound, s.active0);
    L.exhausted = true;
  }
  if (s.work >= G && s.active0 <= finish_paths) {
    L.finished = true;
    return s.active0 > 0 ? LoopStep::kHandOff : LoopStep::kFinished;
  }
  return LoopStep::kGoOn;
}

}  // namespace mrt
