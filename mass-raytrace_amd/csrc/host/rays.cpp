// rays.cpp — the host-only half of mrt_render_rays (include/massrt.h): the
// published path stream and the renderer's own camera rays as table entries.
// Plain C++ over mrt_rng.h and the kernels' camera code (material.h
// camera_ray, compiled here for the host: the same source, IEEE f32 in the
// same order, no contraction), no HIP and no context.
#include <string>

#include "../device/material.h"

using namespace mrt;

// errors without a context (api.hip)
__attribute__((visibility("hidden"))) extern thread_local std::string mrt_global_error;

namespace {

int invalid(const char* msg) {
  mrt_global_error = msg;
  return MRT_ERR_INVALID;
}

}  // namespace

extern "C" {

int mrt_path_stream(uint64_t seed, uint32_t key, uint32_t sample, uint32_t n, uint64_t* out_u64, float* out_f32) {
  PathRng rng = path_rng(seed, key, sample);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t r = rng.next();
    if (out_u64) out_u64[i] = r;
    if (out_f32) out_f32[i] = bits_to_unit_f32((uint32_t)(r >> 32));  // PathRng::f32 of that draw
  }
  return MRT_OK;
}

int mrt_camera_rays(const mrt_camera* camera, uint32_t width, uint32_t height, const uint32_t* pixels, uint32_t n,
                    uint64_t seed, uint32_t sample, mrt_path_ray* out) {
  if (!camera) return invalid("mrt_camera_rays: null camera");
  if (width == 0 || height == 0 || (uint64_t)width * height >= (1ull << 32))
    return invalid("mrt_camera_rays: bad image size");
  if (n && (!pixels || !out)) return invalid("mrt_camera_rays: null pixels or output");
  const uint32_t n_pix = width * height;
  for (uint32_t j = 0; j < n; ++j)
    if (pixels[j] >= n_pix) return invalid("mrt_camera_rays: pixel outside the image");
  DevCamera cam;
  cam.origin = ld3(camera->origin);
  cam.llc = ld3(camera->lower_left_corner);
  cam.horizontal = ld3(camera->horizontal);
  cam.vertical = ld3(camera->vertical);
  cam.u = ld3(camera->u);
  cam.v = ld3(camera->v);
  cam.lens_radius = camera->lens_radius;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t p = pixels[j], y = p / width, x = p - y * width;
    PathRng rng = path_rng(seed, p, sample);
    V3 o, d;
    camera_ray(cam, x, y, width, height, rng, o, d);
    // the draws camera_ray took: a fresh copy of the stream steps until it
    // stands where the ray left it (2 for the jitter + 2 per disk try)
    PathRng walk = path_rng(seed, p, sample);
    uint32_t skip = 0;
    while ((walk.s0 != rng.s0 || walk.s1 != rng.s1) && skip <= MRT_RAY_SKIP_MAX) walk.next(), ++skip;
    if (skip > MRT_RAY_SKIP_MAX) return invalid("mrt_camera_rays: a ray took more than MRT_RAY_SKIP_MAX draws");
    out[j] = mrt_path_ray{{o.x, o.y, o.z}, {d.x, d.y, d.z}, p, skip};
  }
  return MRT_OK;
}

}  // extern "C"
