// rays_check — the work items and limits of a caller's ray list
// (mrt_render_rays) on the host (csrc/host/loop.h), for tests/test_rays.py.
// Prints cases; the test asserts.
//   rays_check work
//     "work spp g i s" (ray_work) for spp in {1, 3, 5, 16, 1024} and g around
//     0, the multiples of spp and the top of the 32-bit range.
//   rays_check skip
//     "clamp skip drawn" (ray_skip) around MRT_RAY_SKIP_MAX, and
//     "bad n first" (first_bad_skip) over tables with the offending entry
//     first, last, twice and absent.
//   rays_check fit
//     "fit spp_begin spp_count 0|1" (samples_fit) around 2^32.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/massrt.h"
#include "../mass-raytrace_amd/csrc/host/loop.h"

using namespace mrt;

static_assert(kRaySkipMax == MRT_RAY_SKIP_MAX, "loop.h clamps to the ABI's limit");

static int work() {
  const uint32_t spps[] = {1, 3, 5, 16, 1024};
  for (uint32_t spp : spps) {
    std::vector<uint32_t> gs = {0, 1, spp - 1, spp, spp + 1, 7 * spp - 1, 7 * spp, 0x7FFFFFFFu, 0x80000000u,
                                0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t g : gs) {
      const RayWork w = ray_work(g, spp);
      printf("work %u %u %u %u\n", spp, g, w.i, w.s);
    }
  }
  return 0;
}

static int skip() {
  const uint32_t skips[] = {0, 1, 2, 4, MRT_RAY_SKIP_MAX - 1, MRT_RAY_SKIP_MAX, MRT_RAY_SKIP_MAX + 1, 0x7FFFFFFFu,
                            0xFFFFFFFFu};
  for (uint32_t s : skips) printf("clamp %u %u\n", s, ray_skip(s));
  // tables of 5 entries; the listed positions hold a skip above the limit
  const std::vector<std::vector<uint32_t>> bad = {{}, {0}, {4}, {2, 3}, {0, 4}};
  for (const auto& at : bad) {
    std::vector<mrt_path_ray> t(5);
    for (uint32_t i = 0; i < 5; ++i) t[i] = mrt_path_ray{{0, 0, 0}, {0, 0, 1}, i, i == 1 ? MRT_RAY_SKIP_MAX : i};
    for (uint32_t i : at) t[i].skip = MRT_RAY_SKIP_MAX + 1 + i;
    printf("bad %zu %u\n", at.size(), first_bad_skip(t.data(), (uint32_t)t.size()));
  }
  printf("bad 0 %u\n", first_bad_skip((const mrt_path_ray*)nullptr, 0u));  // an empty table: none
  return 0;
}

static int fit() {
  const uint32_t cases[][2] = {{0, 0},          {0, 1},          {0, 0xFFFFFFFFu}, {1, 0xFFFFFFFEu}, {1, 0xFFFFFFFFu},
                               {0xFFFFFFFFu, 0}, {0xFFFFFFFFu, 1}, {0x80000000u, 0x7FFFFFFFu},
                               {0x80000000u, 0x80000000u}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
  for (auto& c : cases) printf("fit %u %u %d\n", c[0], c[1], samples_fit(c[0], c[1]) ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "work")) return work();
  if (argc == 2 && !strcmp(argv[1], "skip")) return skip();
  if (argc == 2 && !strcmp(argv[1], "fit")) return fit();
  fprintf(stderr, "usage: rays_check work|skip|fit\n");
  return 2;
}
