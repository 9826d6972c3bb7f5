// views_check — the pixel lists of a batch of views (mrt_render_views) on the
// host (csrc/host/loop.h), for tests/test_views.py. Prints cases; the test
// asserts.
//   views_check lists
//     for W x H in {2x2, 9x7, 21x13, 131x75}, V in {1, 2, 5}, shard_count in
//     {1, 3} and every shard: "shard W H sc si p.." (shard_list, tile 8),
//     "views W H V sc si P.." (view_list over it) and "split W H V sc si v:p.."
//     (view_split of every entry of the views line, in its order).
//   views_check limit
//     "fit n_views W H 0|1" (views_fit) around n_views W H = 2^32.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/massrt.h"
#include "../mass-raytrace_amd/csrc/host/loop.h"

using namespace mrt;

static int lists() {
  const uint32_t sizes[][2] = {{2, 2}, {9, 7}, {21, 13}, {131, 75}};
  const uint32_t views[] = {1, 2, 5}, shards[] = {1, 3};
  for (auto& wh : sizes)
    for (uint32_t sc : shards)
      for (uint32_t si = 0; si < sc; ++si) {
        const uint32_t W = wh[0], H = wh[1];
        const std::vector<uint32_t> shard = shard_list(W, H, si, sc, MRT_TILE);
        printf("shard %u %u %u %u", W, H, sc, si);
        for (uint32_t p : shard) printf(" %u", p);
        printf("\n");
        for (uint32_t V : views) {
          const std::vector<uint32_t> list = view_list(shard, V, W * H);
          printf("views %u %u %u %u %u", W, H, V, sc, si);
          for (uint32_t P : list) printf(" %u", P);
          printf("\nsplit %u %u %u %u %u", W, H, V, sc, si);
          for (uint32_t P : list) {
            const ViewPixel vp = view_split(P, W * H);
            printf(" %u:%u", vp.v, vp.p);
          }
          printf("\n");
        }
      }
  return 0;
}

static int limit() {
  const uint64_t cases[][3] = {
      {1, 65535, 65537},  // 2^32 - 1
      {1, 65536, 65536},  // 2^32
      {2, 65536, 32768},  // 2^32
      {3, 21845, 65537},  // 3 * 1431655765 = 2^32 - 1
      {4, 32768, 32768},  // 2^32
      {4, 32768, 32767},  // 2^32 - 2^17
      {0xFFFFFFFFull, 1, 1},
      {0x100000000ull, 1, 1},
      {0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull},  // the 64-bit products must not wrap into range
      {0x100000001ull, 0xFFFFFFFFull, 1},
      {0, 4, 4},
      {1, 0, 4},
      {1, 4, 0},
      {5, 21, 13},
  };
  for (auto& c : cases)
    printf("fit %llu %llu %llu %d\n", (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2],
           views_fit(c[0], (uint32_t)c[1], (uint32_t)c[2]) ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "lists")) return lists();
  if (argc == 2 && !strcmp(argv[1], "limit")) return limit();
  fprintf(stderr, "usage: views_check lists|limit\n");
  return 2;
}
