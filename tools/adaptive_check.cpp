// adaptive_check — the round schedule and the argument checks of
// mrt_render_adaptive on the host (csrc/host/adaptive.h: the functions the
// library's host loop calls), for tests/test_adaptive.py. Prints; the test asserts.
//   adaptive_check rounds MIN STEP CAP
//     "round r first count" for every round of a call in which no tile closes
//     (adapt_round_count, adapt_goes_on), then "limit n" (adapt_round_limit).
//   adaptive_check args MIN STEP THRESHOLD FLOOR SPP_BEGIN SPP_COUNT FLAGS
//     "ok", or "error <text>" (adapt_render_error); THRESHOLD and FLOOR as
//     strtof reads them ("nan", "inf", "-1").
//   adaptive_check slots
//     "slot x y i" (adapt_slot) over a 17 x 9 patch, and "tiles W H si sc n"
//     (adapt_shard_tiles) for a few frames and shards.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/massrt.h"
#include "../mass-raytrace_amd/csrc/host/adaptive.h"

using namespace mrt;

static int rounds(uint32_t mn, uint32_t step, uint32_t cap) {
  const mrt_adaptive_params p{mn, step, 0.0f, 0.0f};
  uint32_t done = 0;
  for (uint32_t r = 0;; ++r) {
    const uint32_t n = adapt_round_count(p, cap, r, done);
    printf("round %u %u %u\n", r, done, n);
    done += n;
    if (!adapt_goes_on(1u, done, cap)) break;
  }
  printf("limit %llu\n", (unsigned long long)adapt_round_limit(p, cap));
  return 0;
}

static int args(char** v) {
  const mrt_adaptive_params p{(uint32_t)strtoul(v[0], nullptr, 0), (uint32_t)strtoul(v[1], nullptr, 0),
                              strtof(v[2], nullptr), strtof(v[3], nullptr)};
  const char* why = adapt_render_error(&p, (uint32_t)strtoul(v[4], nullptr, 0), (uint32_t)strtoul(v[5], nullptr, 0),
                                       (uint32_t)strtoul(v[6], nullptr, 0));
  if (why)
    printf("error %s\n", why);
  else
    printf("ok\n");
  return 0;
}

static int slots() {
  for (uint32_t y = 0; y < 9; ++y)
    for (uint32_t x = 0; x < 17; ++x) printf("slot %u %u %u\n", x, y, adapt_slot(x, y));
  const uint32_t cases[][4] = {{50, 27, 0, 1}, {50, 27, 0, 3}, {50, 27, 2, 3}, {8, 8, 0, 1}, {1, 1, 0, 1},
                               {9, 17, 3, 4},  {9, 17, 7, 8},  {1, 1, 1, 2},   {1920, 1080, 0, 1}};
  for (auto& c : cases) printf("tiles %u %u %u %u %u\n", c[0], c[1], c[2], c[3], adapt_shard_tiles(c[0], c[1], c[2], c[3]));
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "rounds"))
    return rounds((uint32_t)strtoul(argv[2], nullptr, 0), (uint32_t)strtoul(argv[3], nullptr, 0),
                  (uint32_t)strtoul(argv[4], nullptr, 0));
  if (argc == 9 && !strcmp(argv[1], "args")) return args(argv + 2);
  if (argc == 2 && !strcmp(argv[1], "slots")) return slots();
  fprintf(stderr, "usage: adaptive_check rounds MIN STEP CAP | args MIN STEP THRESHOLD FLOOR BEGIN COUNT FLAGS | slots\n");
  return 2;
}
