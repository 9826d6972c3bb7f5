// volume_check — volumes whose boundary is an instance or a model, on the host,
// no GPU needed: a world given on the command line through the builder calls
// (mrt_builder_add_volume_instance / _model, mrt_builder_add_sphere), uploaded
// as mrt_upload_scene_targets does (build_host_scene with the target table),
// and walked by the device headers' own closest_hit<COUNT, RNG> (walk.h,
// compiled here for the host: the same source, the same bits), one ray at a
// time, each with the stream mrt_trace_rays gives it (seed 0, ray i, sample
// 0xFFFFFFFE). tests/test_volume_targets.py compares what it writes with a
// composition over the CPU oracle.
//   hipcc --offload-host-only -x hip -O2 -std=c++17 -ffp-contract=off -fno-fast-math -o volume_check
//       tools/volume_check.cpp -Lmass-raytrace_amd/massrt -lmassrt -Wl,-rpath,$PWD/mass-raytrace_amd/massrt
//   (plain g++ -O2 -std=c++17 -ffp-contract=off builds it too)
//   volume_check <cube.ply> <t_min> <t_max> <rays.f32> <out.u32> [build] <object>...
//     objects, added to the world in this order (World::add; no build_bvh unless `build` is given):
//       sphere <cx> <cy> <cz> <r>                                  a Lambertian sphere
//       vinst <density> <tx> <ty> <tz> <rx> <ry> <rz> <sx> <sy> <sz>  Volume(model.instance(t, r, s), density, albedo 1)
//       vmodel <density>                                            Volume(model, density, albedo 1)
//       vsphere <cx> <cy> <cz> <r> <density>                        Volume(Sphere, density, albedo 1)
//     and, for the validation checks (a rejected scene prints `invalid: <message>` and exits with 4):
//       target <volume> <kind> <index>   one more mrt_volume_target entry, as given
//       blas-sphere                      the model's first triangle leaf replaced by sphere 0
//     rays: n x 6 float32; out: n x 4 uint32 {prim, container, t bits (0: no hit), 0}
//     stdout: the counters summed over the rays, `name value` pairs on one line
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../mass-raytrace_amd/csrc/device/upload.h"
#include "../mass-raytrace_amd/csrc/device/walk.h"

using namespace mrt;

namespace {

int usage() {
  fprintf(stderr, "volume_check <cube.ply> <t_min> <t_max> <rays.f32> <out.u32> [build] <object>...\n");
  return 1;
}

int builder_fail(const char* what) {
  fprintf(stderr, "%s: %s\n", what, mrt_builder_last_error());
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 7) return usage();
  const float tmin = strtof(argv[2], nullptr), tmax = strtof(argv[3], nullptr);
  mrt_builder* b = nullptr;
  mrt_builder_new(1, &b);
  const int lam = mrt_builder_material(b, MRT_MAT_LAMBERTIAN, (uint32_t)mrt_builder_solid(b, 0.5f, 0.5f, 0.5f, 1.0f), 0, 0, 0, 0);
  const int none = mrt_builder_material(b, MRT_MAT_NONE, 0, 0, 0, 0, 0);
  if (lam < 0 || none < 0) return builder_fail("material");
  const int model = mrt_builder_model_from_ply(b, argv[1], (uint32_t)none, MRT_NO_MATERIAL, 0);
  if (model < 0) return builder_fail(argv[1]);
  const float white[3] = {1, 1, 1};
  bool build = false, blas_sphere = false;
  std::vector<mrt_volume_target> raw_targets;
  for (int a = 6; a < argc;) {
    const std::string kind = argv[a++];
    auto take = [&](int n, float* out) {
      if (a + n > argc) return false;
      for (int k = 0; k < n; ++k) out[k] = strtof(argv[a++], nullptr);
      return true;
    };
    float v[10];
    int rc;
    if (kind == "build") {
      build = true;
      continue;
    } else if (kind == "blas-sphere") {
      blas_sphere = true;
      continue;
    } else if (kind == "target") {
      if (!take(3, v)) return usage();
      raw_targets.push_back(mrt_volume_target{(uint32_t)v[0], MRT_REF((uint32_t)v[1], (uint32_t)v[2])});
      continue;
    } else if (kind == "vsphere") {
      if (!take(5, v)) return usage();
      rc = mrt_builder_add_volume(b, v, v[3], v[4], white);
    } else if (kind == "sphere") {
      if (!take(4, v)) return usage();
      rc = mrt_builder_add_sphere(b, (uint32_t)lam, v[0], v[1], v[2], v[3]);
    } else if (kind == "vinst") {
      if (!take(10, v)) return usage();
      rc = mrt_builder_add_volume_instance(b, model, v + 1, v + 4, v + 7, v[0], white);
    } else if (kind == "vmodel") {
      if (!take(1, v)) return usage();
      rc = mrt_builder_add_volume_model(b, model, v[0], white);
    } else {
      return usage();
    }
    if (rc < 0) return builder_fail(kind.c_str());
  }
  if (build && mrt_builder_build_bvh(b) != MRT_OK) return builder_fail("build_bvh");
  mrt_scene_desc d;
  const mrt_volume_target* targets = nullptr;
  uint32_t n_targets = 0;
  if (mrt_builder_desc(b, &d, nullptr) != MRT_OK || mrt_builder_volume_targets(b, &targets, &n_targets) != MRT_OK)
    return builder_fail("desc");
  // the malformed tables of the validation checks: entries as given, after the builder's own
  std::vector<mrt_volume_target> table(targets, targets + n_targets);
  table.insert(table.end(), raw_targets.begin(), raw_targets.end());
  std::vector<mrt_node> nodes(d.nodes, d.nodes + d.n_nodes);
  if (blas_sphere) {  // the model's first leaf becomes a sphere: a BLAS no volume may have as its target
    for (mrt_node& nd : nodes)
      if (MRT_REF_KIND(nd.left) == MRT_REF_TRIANGLE) {
        nd.left = MRT_REF(MRT_REF_SPHERE, 0);
        break;
      }
    d.nodes = nodes.data();
  }
  HostScene s;
  s.nf_build = kNfBuildNever;
  std::string err;
  if (!build_host_scene(d, s, err, true, nullptr, table.data(), (uint32_t)table.size())) {
    printf("invalid: %s\n", err.c_str());
    mrt_builder_free(b);
    return 4;
  }
  const DevScene S = host_dev_scene(s);

  FILE* f = fopen(argv[4], "rb");
  if (!f) return fprintf(stderr, "cannot read %s\n", argv[4]), 1;
  std::vector<float> rays;
  float buf[6 * 1024];
  for (size_t k; (k = fread(buf, sizeof(float), 6 * 1024, f)) > 0;) rays.insert(rays.end(), buf, buf + k);
  fclose(f);
  const size_t n = rays.size() / 6;
  std::vector<uint32_t> out(4 * n);
  uint64_t node_visits = 0, triangle_tests = 0, sphere_tests = 0, instance_entries = 0, model_entries = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* r = &rays[6 * i];
    // a one-ray pool (k_rays_in's slot 0) and the walk's inputs over it
    const float4 ro = make_float4(r[0], r[1], r[2], 0.0f), rd = make_float4(r[3], r[4], r[5], 0.0f);
    const TravIn in{S, reinterpret_cast<const uint4*>(S.slots), S.world_begin, &ro, &rd, tmin};
    PathRng rng = path_rng(0, (uint32_t)i, 0xFFFFFFFEu);
    LocalCounters lc;
    const Hit h = closest_hit<true, true>(in, 0, tmax, lc, rng);
    const bool hit = h.prim != kRefNone;
    uint32_t tb;
    memcpy(&tb, &h.t, 4);
    out[4 * i] = h.prim;
    out[4 * i + 1] = h.container;
    out[4 * i + 2] = hit ? tb : 0u;
    out[4 * i + 3] = 0;
    node_visits += lc.node_visits, triangle_tests += lc.triangle_tests, sphere_tests += lc.sphere_tests;
    instance_entries += lc.instance_entries, model_entries += lc.model_entries;
  }
  f = fopen(argv[5], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return fprintf(stderr, "cannot write %s\n", argv[5]), 1;
  fclose(f);
  printf("node_visits %llu triangle_tests %llu sphere_tests %llu instance_entries %llu model_entries %llu\n",
         (unsigned long long)node_visits, (unsigned long long)triangle_tests, (unsigned long long)sphere_tests,
         (unsigned long long)instance_entries, (unsigned long long)model_entries);
  mrt_builder_free(b);
  return 0;
}
