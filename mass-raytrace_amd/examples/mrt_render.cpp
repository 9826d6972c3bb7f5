// mrt_render — the C++ driver in the role of the reference's render()
// (main.rs:150-295) + export (main.rs:760-783), written against the C ABI
// only (include/massrt.h): build a built-in Scene, pre-pass, render N
// passes of 1 spp into the accumulation buffers, tonemap, write PNGs
// (<out>.png, <out>_depth.png, _albedo, _normal and _denoise).
//
//   mrt_render [--orbit N | --pano W H | --adaptive T] <scene> <width> <height> <passes> <out.png> [asset_dir] [device]
//
// --orbit N: the reference's EXPORT_FRAMES loop (main.rs:104-141) for a world
// that does not change: N cameras on a circle around the built-in camera's
// look_at, all rendered by ONE mrt_render_views call, each view's slice
// tonemapped and written as frame_%05d.png next to <out.png> (which is not
// written).
//
// --pano W H: a camera model the library does not have, through
// mrt_render_rays: an equirectangular 360-degree frame of W x H pixels from the
// built-in camera's look_from, written to <out.png> (the <width> <height> of
// the command line are not used). The rays are built here on the host, one
// per pixel through its centre, key = the pixel, skip = 0; host buffers, then
// mrt_tonemap and mrt_write_png.
//
// --adaptive T: <passes> is a cap, not a count: mrt_render_adaptive samples every
// 8x8 tile in rounds until its error estimate is below T of its brightness
// (the library's default minimum, step and floor) or the cap is spent. Writes
// the resolved frame to <out.png> and the sample map to <out>_samples.png
// (white: the tiles that took the most samples).
//
// Prints one line: scene, size, passes, render seconds, Msamples/s.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/massrt.h"

static int fail(const char* what, mrt_ctx* ctx) {
  std::fprintf(stderr, "%s failed: %s\n", what, ctx ? mrt_last_error(ctx) : mrt_global_last_error());
  return 1;
}

// The built-in camera turned about the vertical axis through its look_at, in
// n steps: Camera::new (world.rs:5-51) run backwards for what it was made
// from (every built-in focuses on its look_at), then mrt_builder_camera.
static bool orbit_views(mrt_builder* b, const mrt_camera& cam, uint32_t n, std::vector<mrt_view>& views) {
  float at[3], from[3], up[3] = {0, 1, 0}, len2 = 0, vert2 = 0;
  for (int k = 0; k < 3; ++k) {
    at[k] = cam.lower_left_corner[k] + 0.5f * cam.horizontal[k] + 0.5f * cam.vertical[k];  // origin - focus w
    len2 += (cam.origin[k] - at[k]) * (cam.origin[k] - at[k]);
    vert2 += cam.vertical[k] * cam.vertical[k];
  }
  const float focus = std::sqrt(len2);
  const float vfov = 2.0f * std::atan(0.5f * std::sqrt(vert2) / focus) * 180.0f / 3.14159265358979f;
  const float hor2 = std::sqrt(cam.horizontal[0] * cam.horizontal[0] + cam.horizontal[1] * cam.horizontal[1] +
                               cam.horizontal[2] * cam.horizontal[2]);
  const float aspect = hor2 / std::sqrt(vert2);
  const float dx = cam.origin[0] - at[0], dz = cam.origin[2] - at[2];
  for (uint32_t v = 0; v < n; ++v) {
    const float phi = 6.28318530717959f * (float)v / (float)n;
    from[0] = at[0] + dx * std::cos(phi) + dz * std::sin(phi);
    from[1] = cam.origin[1];
    from[2] = at[2] - dx * std::sin(phi) + dz * std::cos(phi);
    mrt_view view;
    if (mrt_builder_camera(b, vfov, from, at, up, aspect, 2.0f * cam.lens_radius, focus) < 0 ||
        mrt_builder_desc(b, nullptr, &view.camera) != MRT_OK)
      return false;
    view.seed = 1 + v;  // frames never share samples (main.rs:167-250: a fresh stream per render)
    views.push_back(view);
  }
  return true;
}

// One ray per pixel of a W x H equirectangular frame around `from`: column x
// is the longitude (the frame's centre looks down -z, x grows to the right),
// row y the latitude, y = 0 the bottom row as in every accumulation buffer.
static std::vector<mrt_path_ray> pano_rays(const float* from, uint32_t W, uint32_t H) {
  std::vector<mrt_path_ray> rays((size_t)W * H);
  for (uint32_t y = 0; y < H; ++y)
    for (uint32_t x = 0; x < W; ++x) {
      const float lon = (((float)x + 0.5f) / (float)W - 0.5f) * 6.28318530717959f;
      const float lat = (((float)y + 0.5f) / (float)H - 0.5f) * 3.14159265358979f;
      mrt_path_ray& r = rays[(size_t)y * W + x];
      for (int k = 0; k < 3; ++k) r.origin[k] = from[k];
      r.direction[0] = std::cos(lat) * std::sin(lon);
      r.direction[1] = std::sin(lat);
      r.direction[2] = -std::cos(lat) * std::cos(lon);
      r.key = y * W + x;  // the pixel's own stream, as a frame's pixel has
      r.skip = 0;         // no draw went into the ray
    }
  return rays;
}

int main(int argc, char** argv) {
  uint32_t orbit = 0, pano_w = 0, pano_h = 0;
  float adaptive = -1.0f;
  for (int i = 1; i + 1 < argc; ++i)
    if (!std::strcmp(argv[i], "--adaptive")) {
      adaptive = (float)std::atof(argv[i + 1]);
      for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
      argc -= 2;
      break;
    } else if (!std::strcmp(argv[i], "--orbit")) {
      orbit = (uint32_t)std::atoi(argv[i + 1]);
      for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
      argc -= 2;
      break;
    } else if (!std::strcmp(argv[i], "--pano") && i + 2 < argc) {
      pano_w = (uint32_t)std::atoi(argv[i + 1]);
      pano_h = (uint32_t)std::atoi(argv[i + 2]);
      for (int j = i; j + 3 < argc; ++j) argv[j] = argv[j + 3];
      argc -= 3;
      break;
    }
  if (argc < 6) {
    std::fprintf(stderr,
                 "usage: %s [--orbit N | --pano W H | --adaptive T] <scene> <width> <height> <passes> <out.png> [asset_dir] [device]\n",
                 argv[0]);
    return 2;
  }
  const std::string scene = argv[1];
  const uint32_t W = (uint32_t)std::atoi(argv[2]), H = (uint32_t)std::atoi(argv[3]);
  const uint32_t passes = (uint32_t)std::atoi(argv[4]);
  const std::string out = argv[5];
  const std::string assets = argc > 6 ? argv[6] : "";
  const int device = argc > 7 ? std::atoi(argv[7]) : 0;

  // Scene::generate + World::build_bvh (scenes.rs, world.rs:117-122); fastrand seed 1 (main.rs:86)
  mrt_builder* b = nullptr;
  if (mrt_builder_new(1, &b) != MRT_OK) return fail("mrt_builder_new", nullptr);
  if (mrt_builder_builtin(b, scene.c_str(), 16.0f / 9.0f, assets.c_str()) < 0) {
    std::fprintf(stderr, "scene: %s\n", mrt_builder_last_error());
    return 1;
  }
  mrt_scene_desc desc;
  mrt_camera cam;
  if (mrt_builder_desc(b, &desc, &cam) != MRT_OK) {
    std::fprintf(stderr, "desc: %s\n", mrt_builder_last_error());
    return 1;
  }
  mrt_ctx* ctx = nullptr;
  if (mrt_create(device, &ctx) != MRT_OK) return fail("mrt_create", nullptr);
  mrt_scene_ext ext;  // the Eve table, empty for the other scenes
  if (mrt_builder_desc_ext(b, &ext) != MRT_OK) {
    std::fprintf(stderr, "desc_ext: %s\n", mrt_builder_last_error());
    return 1;
  }
  const mrt_volume_target* targets = nullptr;  // the fog boxes' boundaries, none for the other scenes
  uint32_t n_targets = 0;
  if (mrt_builder_volume_targets(b, &targets, &n_targets) != MRT_OK) {
    std::fprintf(stderr, "volume_targets: %s\n", mrt_builder_last_error());
    return 1;
  }
  if (mrt_upload_scene_targets(ctx, &desc, &ext, targets, n_targets) != MRT_OK)
    return fail("mrt_upload_scene_targets", ctx);
  if (mrt_set_camera(ctx, &cam) != MRT_OK) return fail("mrt_set_camera", ctx);

  if (pano_w && pano_h) {
    mrt_builder_free(b);
    const std::vector<mrt_path_ray> rays = pano_rays(cam.origin, pano_w, pano_h);  // lens_radius 0: origin = look_from
    std::vector<float> rgb(rays.size() * 3, 0.0f);
    std::vector<uint32_t> bounces(rays.size(), 0);
    std::vector<uint8_t> bytes(rays.size() * 3);
    const auto t0 = std::chrono::steady_clock::now();
    if (mrt_render_rays(ctx, rays.data(), (uint32_t)rays.size(), 1, 0, passes, 50, 0, rgb.data(), bounces.data()) !=
        MRT_OK)
      return fail("mrt_render_rays", ctx);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // entry y*W + x is pixel (x, y) of an ordinary W x H frame
    if (mrt_tonemap(ctx, pano_w, pano_h, rgb.data(), bounces.data(), passes, MRT_DISPLAY_DEFAULT, bytes.data()) != MRT_OK)
      return fail("mrt_tonemap", ctx);
    if (mrt_write_png(out.c_str(), pano_w, pano_h, bytes.data()) != MRT_OK) {
      std::fprintf(stderr, "png: %s\n", mrt_builder_last_error());
      return 1;
    }
    std::printf("%s pano %ux%u passes=%u render_s=%.3f msamples_per_s=%.1f\n", scene.c_str(), pano_w, pano_h, passes,
                secs, (double)rays.size() * passes / secs / 1e6);
    mrt_destroy(ctx);
    return 0;
  }
  const size_t n = (size_t)W * H;
  if (orbit) {
    std::vector<mrt_view> views;
    if (!orbit_views(b, cam, orbit, views)) {
      std::fprintf(stderr, "camera: %s\n", mrt_builder_last_error());
      return 1;
    }
    mrt_builder_free(b);
    std::vector<float> rgb(n * 3 * orbit, 0.0f);
    std::vector<uint32_t> bounces(n * orbit, 0);
    std::vector<uint8_t> bytes(n * 3);
    const auto t0 = std::chrono::steady_clock::now();
    mrt_render_args a{W, H, 0, passes, 0, 50, 0, 1, 0};  // the seeds are the views'
    if (mrt_render_views(ctx, &a, views.data(), orbit, rgb.data(), bounces.data()) != MRT_OK)
      return fail("mrt_render_views", ctx);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const size_t slash = out.rfind('/');
    const std::string dir = slash == std::string::npos ? "" : out.substr(0, slash + 1);
    for (uint32_t v = 0; v < orbit; ++v) {  // a view's slice is an ordinary W x H frame
      if (mrt_tonemap(ctx, W, H, rgb.data() + v * n * 3, bounces.data() + v * n, passes, MRT_DISPLAY_DEFAULT,
                      bytes.data()) != MRT_OK)
        return fail("mrt_tonemap", ctx);
      char name[32];
      std::snprintf(name, sizeof name, "frame_%05u.png", v);
      if (mrt_write_png((dir + name).c_str(), W, H, bytes.data()) != MRT_OK) {
        std::fprintf(stderr, "png: %s\n", mrt_builder_last_error());
        return 1;
      }
    }
    std::printf("%s %ux%u views=%u passes=%u render_s=%.3f msamples_per_s=%.1f\n", scene.c_str(), W, H, orbit, passes,
                secs, (double)n * orbit * passes / secs / 1e6);
    mrt_destroy(ctx);
    return 0;
  }
  if (adaptive >= 0.0f) {
    mrt_builder_free(b);
    std::vector<float> rgb(n * 3, 0.0f), moments(n * 2, 0.0f), resolved(n * 3);
    std::vector<uint32_t> bounces(n, 0), samples(n, 0);
    std::vector<uint8_t> bytes(n * 3);
    mrt_adaptive_params prm;
    mrt_adaptive_default_params(&prm);
    prm.threshold = adaptive;
    if (prm.min_spp > passes) prm.min_spp = passes;
    mrt_adaptive_report rep;
    const auto t0 = std::chrono::steady_clock::now();
    mrt_render_args a{W, H, 0, passes, 1, 50, 0, 1, 0};
    if (mrt_render_adaptive(ctx, &a, &prm, rgb.data(), bounces.data(), moments.data(), samples.data(), &rep) != MRT_OK)
      return fail("mrt_render_adaptive", ctx);
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (mrt_adaptive_resolve(ctx, W, H, rgb.data(), samples.data(), resolved.data()) != MRT_OK)
      return fail("mrt_adaptive_resolve", ctx);
    const size_t dot = out.rfind('.');
    const std::string map = (dot == std::string::npos ? out : out.substr(0, dot)) + "_samples.png";
    // the resolved means take Default's bytes with passes = 1; the sample map is the Depth view of the counts
    if (mrt_tonemap(ctx, W, H, resolved.data(), samples.data(), 1, MRT_DISPLAY_DEFAULT, bytes.data()) != MRT_OK ||
        mrt_write_png(out.c_str(), W, H, bytes.data()) != MRT_OK ||
        mrt_tonemap(ctx, W, H, resolved.data(), samples.data(), 1, MRT_DISPLAY_DEPTH, bytes.data()) != MRT_OK ||
        mrt_write_png(map.c_str(), W, H, bytes.data()) != MRT_OK)
      return fail("export", ctx);
    std::printf("%s %ux%u adaptive=%g cap=%u rounds=%u mean_spp=%.1f tiles_open=%u/%u render_s=%.3f msamples_per_s=%.1f\n",
                scene.c_str(), W, H, adaptive, passes, rep.rounds, (double)rep.samples / (double)n, rep.tiles_open,
                rep.tiles, secs, (double)rep.samples / secs / 1e6);
    mrt_destroy(ctx);
    return 0;
  }
  mrt_builder_free(b);
  std::vector<float> albedo(n * 3), normal(n * 3), rgb(n * 3, 0.0f);
  std::vector<uint32_t> bounces(n, 0);
  std::vector<uint8_t> bytes(n * 3);
  // pre-render pass (main.rs:162-222)
  if (mrt_prepass(ctx, W, H, 1, albedo.data(), normal.data()) != MRT_OK) return fail("mrt_prepass", ctx);
  // passes (main.rs:235-290): each pass is one sample of every pixel, merged in order
  const auto t0 = std::chrono::steady_clock::now();
  mrt_render_args a{W, H, 0, passes, 1, 50, 0, 1, 0};
  if (mrt_render(ctx, &a, rgb.data(), bounces.data()) != MRT_OK) return fail("mrt_render", ctx);
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  // export (main.rs:760-783): Default view, plus the auxiliary views next to it
  const char* names[4] = {"", "_depth", "_albedo", "_normal"};
  for (uint32_t mode = MRT_DISPLAY_DEFAULT; mode <= MRT_DISPLAY_NORMAL; ++mode) {
    const float* src = mode == MRT_DISPLAY_ALBEDO ? albedo.data() : mode == MRT_DISPLAY_NORMAL ? normal.data() : rgb.data();
    if (mrt_tonemap(ctx, W, H, src, bounces.data(), passes, mode, bytes.data()) != MRT_OK) return fail("mrt_tonemap", ctx);
    std::string path = out;
    if (mode) {
      const size_t dot = path.rfind('.');
      path = (dot == std::string::npos ? path : path.substr(0, dot)) + names[mode] + ".png";
    }
    if (mrt_write_png(path.c_str(), W, H, bytes.data()) != MRT_OK) {
      std::fprintf(stderr, "png: %s\n", mrt_builder_last_error());
      return 1;
    }
  }
  // the Denoise view (image.dump(.., DisplayMode::Denoise), main.rs:121-127, 675-683): the guided filter over
  // the sums and the pre-pass, then Default's bytes of the filtered colour
  {
    std::vector<float> filtered(n * 3);
    if (mrt_denoise(ctx, W, H, rgb.data(), passes, albedo.data(), normal.data(), nullptr, filtered.data()) != MRT_OK)
      return fail("mrt_denoise", ctx);
    if (mrt_tonemap(ctx, W, H, filtered.data(), bounces.data(), passes ? 1 : 0, MRT_DISPLAY_DEFAULT, bytes.data()) !=
        MRT_OK)
      return fail("mrt_tonemap", ctx);
    const size_t dot = out.rfind('.');
    const std::string path = (dot == std::string::npos ? out : out.substr(0, dot)) + "_denoise.png";
    if (mrt_write_png(path.c_str(), W, H, bytes.data()) != MRT_OK) {
      std::fprintf(stderr, "png: %s\n", mrt_builder_last_error());
      return 1;
    }
  }
  std::printf("%s %ux%u passes=%u render_s=%.3f msamples_per_s=%.1f\n", scene.c_str(), W, H, passes, secs,
              (double)n * passes / secs / 1e6);
  mrt_destroy(ctx);
  return 0;
}
