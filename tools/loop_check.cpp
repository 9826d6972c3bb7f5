// loop_check — the wavefront loop's integer decisions on the host
// (csrc/host/loop.h), for tests/test_loop.py. Prints cases, one per line; the
// test asserts.
//   loop_check refill
//     every cap in 1..10, lo + hi <= cap, G in 1..2 cap + 2 and work counter
//     in 0..G + cap + 1, through k_reserve's steps (the counter is advanced
//     only while it is below G): "cap lo hi G work want gen_slot gen_count
//     gen_base gen_move gen_move_src gen_move_dst active".
//   loop_check sizes
//     "const kPathBytes kPoolFloor", then a grid of renders and budgets
//     through plan_sizes: "plan n_pix spp pool_paths queues budget need_pool P
//     spp_chunk fits pool_bytes(P)", and first_chunk: "chunk spp_count
//     results_max n_pix first".
//   loop_check share
//     queue_share for K in 1..4, P in 1..40 and every n0 <= K ceil(P / K):
//     "K P n0 share_0 .. share_K-1".
//   loop_check status
//     "const kBatch kMaxIterations", then scripted status sequences through
//     on_status, a sequence ending where its queue does: "seq G finish_paths
//     active0 active1 shade_short work step bound exhausted finished" (step:
//     go_on, hand_off, finished or shade_short; bound -1: unbounded).
//   loop_check nothing
//     nothing_to_add over 0, 1, 7 and 2^32 - 1 in each place: "spp_count
//     max_depth n 0|1".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../mass-raytrace_amd/csrc/host/loop.h"

using namespace mrt;

static int refill() {
  for (uint32_t cap = 1; cap <= 10; ++cap)
    for (uint32_t lo = 0; lo <= cap; ++lo)
      for (uint32_t hi = 0; lo + hi <= cap; ++hi)
        for (uint32_t G = 1; G <= 2 * cap + 2; ++G)
          for (uint32_t work = 0; work <= G + cap + 1; ++work) {
            const uint32_t want = refill_want(lo + hi, cap);
            const uint32_t base = want && work < G ? work : G;  // what the atomicAdd returned, if one was issued
            const RefillPlan p = plan_refill(lo, hi, cap, G, base);
            printf("%u %u %u %u %u %u %u %u %u %u %u %u %u\n", cap, lo, hi, G, work, want, p.gen_slot, p.gen_count,
                   p.gen_base, p.gen_move, p.gen_move_src, p.gen_move_dst, p.active);
          }
  return 0;
}

static int sizes() {
  printf("const %zu %zu\n", kPathBytes, kPoolFloor);
  const uint32_t n_pixs[] = {1, 7, 48 * 27, 1920 * 1080, 3840 * 2160};
  const uint32_t spps[] = {1, 3, 64, 1024, 4096};
  const size_t pools[] = {(size_t)1 << 16, ((size_t)64 << 20) - 1, (size_t)64 << 20, ((size_t)64 << 20) + 1,
                          (size_t)100 << 20, (size_t)384 << 20, (size_t)1 << 30};
  for (uint32_t n_pix : n_pixs)
    for (uint32_t spp : spps)
      for (size_t pool : pools)
        for (int K = 1; K <= 4; ++K)
          for (int need_pool = 0; need_pool <= 1; ++need_pool) {
            const size_t P0 = pool_wanted(n_pix, spp, pool, need_pool != 0);
            const size_t all = (P0 ? pool_bytes(K, P0) : 0) + (size_t)n_pix * spp * 16;  // everything fits
            const size_t one = (size_t)n_pix * 16;                                      // one sample per pixel, no pool
            std::vector<size_t> budgets = {0, one - 1, one, one + 4096 * (size_t)K, all - 1, all, all + 1, 2 * all};
            for (int f = 1; f < 16; ++f) budgets.push_back(all / 16 * f);
            for (int s = 0; s < 40; ++s) budgets.push_back(all >> s);
            for (size_t budget : budgets) {
              const SizePlan s = plan_sizes(n_pix, spp, pool, K, budget, need_pool != 0);
              printf("plan %u %u %zu %d %zu %d %zu %u %d %zu\n", n_pix, spp, pool, K, budget, need_pool, s.P, s.spp_chunk,
                     s.fits ? 1 : 0, pool_bytes(K, s.P));
            }
          }
  const uint64_t maxes[] = {1ull << 10, 1000003ull, 1ull << 31};
  const uint32_t counts[] = {1, 2, 5, 1024, 0xFFFFFFFFu};
  for (uint32_t n_pix : {1u, 7u, 1296u, 1u << 10, 1920u * 1080u, 0xFFFFFFFFu})
    for (uint64_t rmax : maxes)
      for (uint32_t spp_count : counts)
        printf("chunk %u %llu %u %u\n", spp_count, (unsigned long long)rmax, n_pix, first_chunk(spp_count, rmax, n_pix));
  return 0;
}

static int share() {
  for (int K = 1; K <= 4; ++K)
    for (uint32_t P = 1; P <= 40; ++P)
      for (uint32_t n0 = 0; n0 <= K * ((P + K - 1) / K); ++n0) {
        printf("%d %u %u", K, P, n0);
        for (int k = 0; k < K; ++k) printf(" %u", queue_share(n0, K, k));
        printf("\n");
      }
  return 0;
}

// One scripted sequence: statuses until the queue finishes or fails.
static void status_seq(int seq, uint32_t G, uint32_t finish_paths, const std::vector<HostStatus>& script) {
  QueueLoop L;
  for (const HostStatus& s : script) {
    const LoopStep r = on_status(L, s, G, finish_paths);
    const char* name = r == LoopStep::kGoOn ? "go_on" : r == LoopStep::kHandOff ? "hand_off" : r == LoopStep::kFinished ? "finished" : "shade_short";
    printf("%d %u %u %u %u %u %u %s %lld %d %d\n", seq, G, finish_paths, s.active0, s.active1, s.shade_short, s.work, name,
           L.bound == ~(size_t)0 ? -1ll : (long long)L.bound, L.exhausted ? 1 : 0, L.finished ? 1 : 0);
    if (r != LoopStep::kGoOn) return;
  }
}

static int status() {
  printf("const %d %u\n", kBatch, kMaxIterations);
  int seq = 0;
  uint32_t rnd = 12345;
  auto next = [&](uint32_t n) {  // LCG, < n
    rnd = rnd * 1664525u + 1013904223u;
    return (rnd >> 8) % n;
  };
  const uint32_t G = 1000, cap = 300;
  for (uint32_t finish_paths : {0u, 1u, 50u, 299u, 300u, 100000u}) {
    // a render as it runs: the pool full while the counter rises, then a drain of random steps down to none
    for (int rep = 0; rep < 8; ++rep) {
      std::vector<HostStatus> sc;
      uint32_t work = cap;
      while (work < G) {
        sc.push_back({cap, cap, 0, work});
        work += 1 + next(cap);
      }
      uint32_t a = cap;
      for (int i = 0; i < 200; ++i) {
        sc.push_back({a, a, 0, work});
        a = a > 0 ? a - std::min(a, 1 + next(1 + a / 2)) : 0;
      }
      status_seq(seq++, G, finish_paths, sc);
    }
    // a live count that rises again after the counter is exhausted (the bound must not follow it up)
    status_seq(seq++, G, finish_paths, {{300, 300, 0, 999}, {280, 0, 0, G}, {290, 0, 0, G}, {120, 0, 0, G + 7}, {200, 0, 0, G + 7}, {60, 0, 0, G + 7}, {0, 0, 0, G + 7}});
    // few paths left while the counter still has work: not finished; then work == G exactly
    status_seq(seq++, G, finish_paths, {{0, 0, 0, 0}, {1, 0, 0, G - 1}, {0, 5, 0, G - 1}, {1, 0, 0, G}, {0, 0, 0, G}});
    // empty at once
    status_seq(seq++, G, finish_paths, {{0, 0, 0, G}});
    // a short k_shade grid fails whatever else the status says
    status_seq(seq++, G, finish_paths, {{300, 300, 0, 10}, {300, 300, 257, 20}});
    status_seq(seq++, G, finish_paths, {{0, 0, 1, G}});
    status_seq(seq++, G, finish_paths, {{10, 0, 0, G}, {5, 0, 4000000000u, G + 1}});
  }
  return 0;
}

static int nothing() {
  const uint32_t vals[] = {0u, 1u, 7u, 0xFFFFFFFFu};
  for (uint32_t spp : vals)
    for (uint32_t depth : vals)
      for (uint32_t n : vals) printf("%u %u %u %d\n", spp, depth, n, nothing_to_add(spp, depth, n) ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "nothing")) return nothing();
  if (!strcmp(mode, "refill")) return refill();
  if (!strcmp(mode, "sizes")) return sizes();
  if (!strcmp(mode, "share")) return share();
  if (!strcmp(mode, "status")) return status();
  return printf("error: expected refill, sizes, share, status or nothing\n"), 2;
}
