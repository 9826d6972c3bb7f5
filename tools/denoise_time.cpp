// denoise_time — how long mrt_denoise_device takes (the Denoise view's guided
// filter, csrc/device/denoise.hip), timed with HIP events on its stream.
//   hipcc -O2 -std=c++17 -o tools/denoise_time tools/denoise_time.cpp \
//     -Lmass-raytrace_amd/massrt -lmassrt -Wl,-rpath,'$ORIGIN/../mass-raytrace_amd/massrt'
//   tools/denoise_time [width height iterations aux runs warmups]     (1920 1080 5 1 20 3)
// For k = 0 .. iterations it times calls of k iterations (`warmups` untimed
// calls, then `runs` calls each between two events) and prints the median;
// the difference of two medians is the iteration at step 2^(k-1) (a call of 0
// iterations only writes the prepared colour out; a call of 1 is the
// preparation plus step 1). The last line is JSON: ms per call at
// `iterations`, per iteration (the mean over steps 2 and up), and the rate
// against the least traffic the filter needs — per pixel 64 B per iteration
// (48 B read with guides, 16 B written; 16 + 16 without) plus the
// preparation's 12 (+24 with guides) B read and 16 (+32) B written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/massrt.h"

#define HIP_OK(x)                                                           \
  do {                                                                      \
    hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                 \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));          \
      return 1;                                                             \
    }                                                                       \
  } while (0)

int main(int argc, char** argv) {
  const uint32_t W = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 1920, H = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 1080;
  const uint32_t iterations = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 5;
  const bool aux = argc > 4 ? std::atoi(argv[4]) != 0 : true;
  const int runs = argc > 5 ? std::atoi(argv[5]) : 20, warmups = argc > 6 ? std::atoi(argv[6]) : 3;
  const size_t n = (size_t)W * H;
  if (n == 0 || iterations > 8 || runs < 1 || warmups < 0) {
    std::fprintf(stderr, "usage: %s [width height iterations<=8 aux runs warmups]\n", argv[0]);
    return 2;
  }
  // a 16-spp-like image: smooth shading under noise, flat albedo regions, a few normals
  std::vector<float> rgb(n * 3), albedo(n * 3), normal(n * 3);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&s] {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(s >> 40) * (1.0f / 16777216.0f);
  };
  const uint32_t passes = 16;
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      const uint32_t region = (x / 97 + 3 * (y / 61)) % 5;
      const float shade = 0.2f + 0.6f * (float)x / (float)W;
      for (int c = 0; c < 3; ++c) {
        albedo[3 * p + c] = 0.2f + 0.15f * (float)((region + c) % 5);
        rgb[3 * p + c] = (float)passes * albedo[3 * p + c] * shade * (0.5f + rnd());
      }
      normal[3 * p] = region == 0 ? 1.0f : 0.0f, normal[3 * p + 1] = region == 1 ? 1.0f : 0.0f;
      normal[3 * p + 2] = region >= 2 && region < 4 ? 1.0f : 0.0f;  // region 4: a miss, zero normal
    }

  mrt_ctx* ctx = nullptr;
  if (mrt_create(0, &ctx) != MRT_OK) {
    std::fprintf(stderr, "mrt_create: %s\n", mrt_global_last_error());
    return 1;
  }
  float *d_rgb, *d_albedo, *d_normal, *d_out;
  HIP_OK(hipMalloc(&d_rgb, n * 12));
  HIP_OK(hipMalloc(&d_albedo, n * 12));
  HIP_OK(hipMalloc(&d_normal, n * 12));
  HIP_OK(hipMalloc(&d_out, n * 12));
  HIP_OK(hipMemcpy(d_rgb, rgb.data(), n * 12, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_albedo, albedo.data(), n * 12, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_normal, normal.data(), n * 12, hipMemcpyHostToDevice));
  hipStream_t st;
  HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  std::vector<hipEvent_t> ev(2 * (size_t)runs);
  for (hipEvent_t& e : ev) HIP_OK(hipEventCreate(&e));

  mrt_denoise_params prm;
  mrt_denoise_default_params(&prm);
  std::vector<double> median(iterations + 1);
  std::vector<float> first(n * 3), again(n * 3);
  for (uint32_t k = 0; k <= iterations; ++k) {
    prm.iterations = k;
    auto call = [&] {
      return mrt_denoise_device(ctx, W, H, d_rgb, passes, aux ? d_albedo : nullptr, aux ? d_normal : nullptr, &prm,
                                d_out, st);
    };
    for (int i = 0; i < warmups; ++i)
      if (call() != MRT_OK) {
        std::fprintf(stderr, "mrt_denoise_device: %s\n", mrt_last_error(ctx));
        return 1;
      }
    HIP_OK(hipStreamSynchronize(st));
    if (k == iterations) HIP_OK(hipMemcpy(first.data(), d_out, n * 12, hipMemcpyDeviceToHost));
    for (int i = 0; i < runs; ++i) {
      HIP_OK(hipEventRecord(ev[2 * i], st));
      if (call() != MRT_OK) {
        std::fprintf(stderr, "mrt_denoise_device: %s\n", mrt_last_error(ctx));
        return 1;
      }
      HIP_OK(hipEventRecord(ev[2 * i + 1], st));
    }
    HIP_OK(hipStreamSynchronize(st));
    std::vector<float> ms((size_t)runs);
    for (int i = 0; i < runs; ++i) HIP_OK(hipEventElapsedTime(&ms[i], ev[2 * i], ev[2 * i + 1]));
    std::sort(ms.begin(), ms.end());
    median[k] = runs % 2 ? ms[runs / 2] : 0.5 * (ms[runs / 2 - 1] + ms[runs / 2]);
    std::printf("iterations %u: median %.4f ms (min %.4f, max %.4f)%s", k, median[k], ms.front(), ms.back(),
                k ? "" : "  [prepared colour written out]\n");
    if (k) std::printf("  step %u: +%.4f ms\n", 1u << (k - 1), median[k] - median[k - 1]);
  }
  // the timed calls computed what the first one did (a checksum ties the figures to a result)
  HIP_OK(hipMemcpy(again.data(), d_out, n * 12, hipMemcpyDeviceToHost));
  double sum = 0;
  bool same = true;
  for (size_t i = 0; i < n * 3; ++i) sum += again[i], same = same && again[i] == first[i];
  const double bytes = (double)n * (64.0 * iterations + (aux ? 36.0 + 48.0 : 12.0 + 16.0));
  const double per_call = median[iterations];
  std::printf(
      "{\"tool\": \"denoise_time\", \"width\": %u, \"height\": %u, \"iterations\": %u, \"aux\": %d, \"runs\": %d, "
      "\"warmups\": %d, \"ms_per_call\": %.4f, \"ms_per_iteration\": %.4f, \"ms_preparation_and_step_1\": %.4f, "
      "\"min_traffic_mb\": %.1f, \"min_traffic_gb_per_s\": %.1f, \"repeatable\": %s, \"mean_out\": %.6f}\n",
      W, H, iterations, aux ? 1 : 0, runs, warmups, per_call,
      iterations > 1 ? (per_call - median[1]) / (iterations - 1) : 0.0, median[iterations ? 1 : 0], bytes / 1e6,
      bytes / (per_call * 1e6),
      same ? "true" : "false", sum / (double)(n * 3));
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(st);
  for (float* d : {d_rgb, d_albedo, d_normal, d_out}) (void)hipFree(d);
  mrt_destroy(ctx);
  return same ? 0 : 1;
}
