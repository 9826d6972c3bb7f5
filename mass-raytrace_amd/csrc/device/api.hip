// api.hip — the context's life behind the C ABI (include/massrt.h): create, destroy,
// scene upload, options and tuning, camera, counters, kernel stats, debug status.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "ctx.h"
#include "upload.h"

using namespace mrt;

__attribute__((visibility("hidden"))) thread_local std::string mrt_global_error;

// ---- the handle of a multi-device context (frames.h) ----------------------
mrt_ctx* ctx_wrap_multi(MultiDev* m) {
  mrt_ctx* c = new mrt_ctx();
  c->multi = m;
  c->device = multi_dev(m, 0)->device;
  return c;
}
MultiDev* ctx_multi(const mrt_ctx* c) { return c ? c->multi : nullptr; }
void ctx_images(mrt_ctx* c, int delta) {
  if (c) c->images += delta;
}
void ctx_set_error(mrt_ctx* c, const std::string& msg) {
  if (c)
    c->err = msg;
  else
    mrt_global_error = msg;
}
int massrt_ctx_device(const mrt_ctx* c) { return c ? c->device : -1; }  // device 0's for a multi-device context

// The ABI's camera as the kernels take it (mrt_set_camera, mrt_render_views).
DevCamera dev_camera(const mrt_camera& cam) {
  DevCamera d;
  d.origin = V3{cam.origin[0], cam.origin[1], cam.origin[2]};
  d.llc = V3{cam.lower_left_corner[0], cam.lower_left_corner[1], cam.lower_left_corner[2]};
  d.horizontal = V3{cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]};
  d.vertical = V3{cam.vertical[0], cam.vertical[1], cam.vertical[2]};
  d.u = V3{cam.u[0], cam.u[1], cam.u[2]};
  d.v = V3{cam.v[0], cam.v[1], cam.v[2]};
  d.lens_radius = cam.lens_radius;
  return d;
}

namespace {

// Re-derives the tuning (options.h derive_tuning) and applies what depends on it in the context.
void apply_options(mrt_ctx* c) {
  const uint32_t wgs_per_cu = c->tun.wgs_per_cu;
  c->tun = derive_tuning(c->opt, c->facts);
  if (c->tun.wgs_per_cu != wgs_per_cu) c->grids.clear();
  c->S.nfb.kmax = ldexpf(1.0f, c->tun.nf_kappa_log2);
}

// Validates and stores option `id`; the caller re-derives (apply_options).
void set_option(mrt_ctx* c, int id, int64_t v) {
  const std::string why = opt_invalid(id, v);
  if (!why.empty()) throw ApiError{MRT_ERR_INVALID, why};
  if (id == OPT_QUEUES && v != c->opt[id] && c->pool.p) {  // the pool is split per queue: reallocated at the next render
    HIP_CHECK(hipDeviceSynchronize());
    release_pool(c);
    c->grids.clear();  // k_trace's grid share depends on the queue count
  }
  c->opt[id] = v;
}

}  // namespace

extern "C" {

int mrt_abi_version(void) { return MRT_ABI_VERSION; }
const char* mrt_global_last_error(void) { return mrt_global_error.c_str(); }
const char* mrt_last_error(const mrt_ctx* c) { return c ? c->err.c_str() : mrt_global_error.c_str(); }

int mrt_create(int device, mrt_ctx** out) {
  if (!out) {
    mrt_global_error = "null output pointer";
    return MRT_ERR_INVALID;
  }
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    mrt_global_error = "no HIP device available (the massrt hot path has no CPU fallback)";
    return MRT_ERR_HIP;
  }
  if (device < 0 || device >= n) {
    mrt_global_error = "device ordinal out of range";
    return MRT_ERR_INVALID;
  }
  mrt_ctx* c = new mrt_ctx();
  c->device = device;
  int rc = guarded(c, [&] {
    HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    for (int i = 0; i < kNumOpts; ++i) c->opt[i] = kOptDefs[i].def;
    apply_options(c);
    for (int k = 0; k < kMaxQueues; ++k) {
      Queue& q = c->q[k];
      HIP_CHECK(hipStreamCreateWithFlags(&q.stream, hipStreamNonBlocking));
      HIP_CHECK(q.ctrl.alloc(1));
      HIP_CHECK(hipHostMalloc(&q.h_stat, 2 * sizeof(HostStatus), hipHostMallocCoherent | hipHostMallocMapped));
      memset(q.h_stat, 0, 2 * sizeof(HostStatus));
      HIP_CHECK(hipHostGetDevicePointer((void**)&q.d_stat, q.h_stat, 0));
      HIP_CHECK(hipEventCreateWithFlags(&q.ev[0], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&q.ev[1], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&q.join, hipEventDisableTiming));
    }
    HIP_CHECK(c->work.alloc(64));  // one 256-byte line
    HIP_CHECK(hipMemset(c->work.p, 0, 256));
    HIP_CHECK(hipEventCreateWithFlags(&c->acc_done, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->set_fork, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->rays_ready, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->ids_ready, hipEventDisableTiming));
    HIP_CHECK(c->d_cnt.alloc(1));
    HIP_CHECK(hipMemset(c->d_cnt.p, 0, sizeof(DevCounters)));
    HIP_CHECK(c->dbg.alloc(4));
    HIP_CHECK(hipMemset(c->dbg.p, 0, 16));
    HIP_CHECK(hipEventCreate(&c->tev[0]));
    HIP_CHECK(hipEventCreate(&c->tev[1]));
    int cus = 0;
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    c->cus = std::max(1, cus);
    c->trace_grid = (uint32_t)c->cus * 4;  // k_trace_simple (debug)
    c->refill_grid = (uint32_t)c->cus * 8;
  });
  if (rc != MRT_OK) {
    mrt_global_error = c->err;
    mrt_destroy(c);
    return rc;
  }
  *out = c;
  return MRT_OK;
}

int mrt_destroy(mrt_ctx* c) {
  if (!c) return MRT_OK;
  if (c->images > 0) {  // an image holds the per-device contexts (massrt.h)
    c->err = "mrt_destroy: " + std::to_string(c->images.load()) + " image(s) of this context still exist";
    mrt_global_error = c->err;
    return MRT_ERR_STATE;
  }
  if (c->multi) {
    multi_free(c->multi);
    delete c;
    return MRT_OK;
  }
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  for (Queue& q : c->q)
    if (q.stream) hipStreamSynchronize(q.stream);
  if (c->acc_done) hipEventDestroy(c->acc_done);
  if (c->set_fork) hipEventDestroy(c->set_fork);
  if (c->rays_ready) hipEventDestroy(c->rays_ready);
  if (c->ids_ready) hipEventDestroy(c->ids_ready);
  if (c->ad_ev) hipEventDestroy(c->ad_ev);
  if (c->ad_words_h) hipHostFree(c->ad_words_h);
  for (Queue& q : c->q) {
    if (q.h_stat) hipHostFree(q.h_stat);
    for (hipEvent_t e : {q.ev[0], q.ev[1], q.join})
      if (e) hipEventDestroy(e);
    if (q.stream) hipStreamDestroy(q.stream);
  }
  if (c->tev[0]) hipEventDestroy(c->tev[0]);
  if (c->tev[1]) hipEventDestroy(c->tev[1]);
  for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;  // the device buffers free themselves (devmem.h), on c->device
  return MRT_OK;
}

int mrt_upload_scene(mrt_ctx* c, const mrt_scene_desc* d) { return mrt_upload_scene_ext(c, d, nullptr); }

int mrt_upload_scene_ext(mrt_ctx* c, const mrt_scene_desc* d, const mrt_scene_ext* ext) {
  return mrt_upload_scene_targets(c, d, ext, nullptr, 0);
}

int mrt_upload_scene_targets(mrt_ctx* c, const mrt_scene_desc* d, const mrt_scene_ext* ext,
                             const mrt_volume_target* targets, uint32_t n_targets) {
  MRT_EACH(c, mrt_upload_scene_targets(c, d, ext, targets, n_targets));
  return guarded(c, [&] {
    if (!d) throw ApiError{MRT_ERR_INVALID, "null scene"};
    HostScene hs;
    std::string err;
    // NF trees per the option in effect at upload (upload.h nf_build)
    hs.nf_build = c->opt[OPT_TRAVERSAL] == MRT_TRAVERSAL_REFERENCE ? kNfBuildNever
                  : c->opt[OPT_TRAVERSAL] == MRT_TRAVERSAL_NEAR_FIRST ? kNfBuildAlways : kNfBuildAuto;
    if (!build_host_scene(*d, hs, err, true, ext, targets, n_targets)) throw ApiError{MRT_ERR_INVALID, err};
    build_treelet(hs, (uint32_t)((size_t)c->tun.treelet_kb * 1024 / 16));
    // one allocation, 256-B aligned sections (upload.h: the arrays' list and their placement)
    const ScenePlan plan = plan_scene(hs);
    HIP_CHECK(c->scene.free());
    c->has_scene = false;
    HIP_CHECK(c->scene.alloc(plan.total + 256));
    DevScene S = host_dev_scene(hs);  // sizes and flags; its pointers now go to the device copies
    size_t k = 0;
    for_each_scene_array(hs, [&](auto field, auto* src, size_t bytes, unsigned flags) {
      char* dst = c->scene.p + plan.off[k++];
      if (bytes) HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
      S.*field = bytes || !(flags & kArrNullIfEmpty) ? (decltype(src))dst : nullptr;
    });
    S.n_tlet = (uint32_t)(hs.tlet.size() / 4);
    S.tl_world_begin = hs.tl_world_begin;
    S.dbg = c->dbg.p;
    c->S = S;
    c->scene_bytes = plan.total;
    // the reference stream's size decides the per-scene rules (the NF trees follow it)
    c->facts.big = (size_t)hs.nf_first_slot * 16 > ((size_t)16 << 20);
    c->facts.instances = S.n_inst;
    c->facts.nf_trees = hs.nf_ok;
    c->facts.treelet = S.n_tlet > 0;
    c->facts.trav_rng = hs.trav_rng;
    c->scene_alpha = hs.has_alpha;
    c->scene_vblas = hs.vol_blas;
    c->scene_ext = !hs.surf_ops.empty() || hs.bg_kind == MRT_BG_CUBEMAP || !hs.eve.empty();
    apply_options(c);  // the per-scene rules of the options left at -1
    c->has_scene = true;
  });
}

int mrt_set_option(mrt_ctx* c, const char* name, int64_t value) {
  if (c && c->multi && name && !strcmp(name, "gather")) return multi_set_gather(c->multi, value, c->err);
  MRT_EACH(c, mrt_set_option(c, name, value));
  return guarded(c, [&] {
    if (name && !strcmp(name, "gather")) {
      if (value != MRT_GATHER_AUTO && value != MRT_GATHER_PEER)
        throw ApiError{MRT_ERR_INVALID, "option gather: a one-device context has no RCCL transport"};
      return;  // nothing to gather on one device
    }
    const int id = opt_find(name);
    if (id < 0) throw ApiError{MRT_ERR_INVALID, std::string("unknown option ") + (name ? name : "(null)")};
    set_option(c, id, value);
    apply_options(c);
  });
}

int mrt_get_option(mrt_ctx* c, const char* name, int64_t* value) {
  if (c && c->multi && name && value && !strcmp(name, "gather")) {
    *value = multi_gather(c->multi);
    return MRT_OK;
  }
  MRT_DEV0(c, mrt_get_option(c, name, value));
  return guarded(c, [&] {
    if (!value) throw ApiError{MRT_ERR_INVALID, "null output"};
    if (name && !strcmp(name, "gather")) {
      *value = MRT_GATHER_AUTO;
      return;
    }
    const int id = opt_find(name);
    if (id < 0) throw ApiError{MRT_ERR_INVALID, std::string("unknown option ") + (name ? name : "(null)")};
    *value = c->opt[id];
  });
}

int mrt_get_tuning(mrt_ctx* c, mrt_tuning* out) {
  MRT_DEV0(c, mrt_get_tuning(c, out));
  return guarded(c, [&] {
    if (!out) throw ApiError{MRT_ERR_INVALID, "null output"};
    const Tuning& t = c->tun;
    out->queues = (uint32_t)t.queues;
    out->trace_refill = t.trace.refill;
    out->trace_box_min = t.trace.box_min;
    out->trace_chunk = t.trace.chunk;
    out->shade_waves = (uint32_t)t.shade_wpe;
    out->pool_paths = t.pool_paths;
    out->results_max = t.results_max;
    out->traversal = t.use_nf ? MRT_TRAVERSAL_NEAR_FIRST : MRT_TRAVERSAL_REFERENCE;
    out->shade_bin = (uint32_t)t.shade_bin;
  });
}

int mrt_scene_device_bytes(mrt_ctx* c, uint64_t* out) {
  MRT_DEV0(c, mrt_scene_device_bytes(c, out));
  return guarded(c, [&] {
    if (!out) throw ApiError{MRT_ERR_INVALID, "null output"};
    *out = c->scene_bytes;
  });
}

int mrt_set_camera(mrt_ctx* c, const mrt_camera* cam) {
  MRT_EACH(c, mrt_set_camera(c, cam));
  return guarded(c, [&] {
    if (!cam) throw ApiError{MRT_ERR_INVALID, "null camera"};
    c->cam = dev_camera(*cam);
    c->has_camera = true;
  });
}

int mrt_get_counters(mrt_ctx* c, mrt_counters* out) {
  if (c && c->multi && out) {  // summed over the devices
    mrt_counters sum{};
    const int rc = on_each(c, [&](mrt_ctx* d) {
      mrt_counters x{};
      const int r = mrt_get_counters(d, &x);
      const uint64_t* px = reinterpret_cast<const uint64_t*>(&x);
      uint64_t* ps = reinterpret_cast<uint64_t*>(&sum);
      for (size_t k = 0; k < sizeof(x) / 8; ++k) ps[k] += px[k];
      return r;
    });
    *out = sum;
    return rc;
  }
  return guarded(c, [&] {
    if (!out) throw ApiError{MRT_ERR_INVALID, "null output"};
    HIP_CHECK(hipStreamSynchronize(c->stream));
    HIP_CHECK(hipDeviceSynchronize());
    DevCounters h;
    HIP_CHECK(hipMemcpy(&h, c->d_cnt.p, sizeof(h), hipMemcpyDeviceToHost));
    out->samples = h.samples;
    out->segments = h.segments;
    out->node_visits = h.node_visits;
    out->sphere_tests = h.sphere_tests;
    out->triangle_tests = h.triangle_tests;
    out->instance_entries = h.instance_entries;
    out->model_entries = h.model_entries;
    out->closest_hits = h.closest_hits;
    out->texel_taps = h.texel_taps;
    out->bounces = h.bounces;
    out->wave_slots = h.wave_slots;
    out->lane_steps = h.lane_steps;
    out->box_exact = h.box_exact;
    out->shaded = h.shaded;
    out->vnf_fallbacks = h.vnf_fallbacks;
    out->shade_waves = h.shade_waves;
    out->shade_kinds = h.shade_kinds;
    out->shade_materials = h.shade_materials;
  });
}

int mrt_reset_counters(mrt_ctx* c) {
  MRT_EACH(c, mrt_reset_counters(c));
  return guarded(c, [&] {
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemset(c->d_cnt.p, 0, sizeof(DevCounters)));
  });
}

int mrt_get_kernel_stats(mrt_ctx* c, mrt_kernel_stats* out) {
  if (c && c->multi && out) {  // summed over the devices
    mrt_kernel_stats sum{};
    const int rc = on_each(c, [&](mrt_ctx* d) {
      mrt_kernel_stats x{};
      const int r = mrt_get_kernel_stats(d, &x);
      sum.trace_ms += x.trace_ms, sum.shade_ms += x.shade_ms, sum.other_ms += x.other_ms;
      sum.trace_launches += x.trace_launches, sum.shade_launches += x.shade_launches;
      sum.iterations += x.iterations, sum.finish_ms += x.finish_ms, sum.finish_launches += x.finish_launches;
      return r;
    });
    *out = sum;
    return rc;
  }
  return guarded(c, [&] {
    if (!out) throw ApiError{MRT_ERR_INVALID, "null output"};
    resolve_kernel_timing(c);
    *out = c->kstats;
  });
}

int mrt_reset_kernel_stats(mrt_ctx* c) {
  MRT_EACH(c, mrt_reset_kernel_stats(c));
  return guarded(c, [&] {
    resolve_kernel_timing(c);
    c->kstats = mrt_kernel_stats{};
  });
}

int mrt_debug_status(mrt_ctx* c, uint32_t* out4) {
  MRT_DEV0(c, mrt_debug_status(c, out4));
  return guarded(c, [&] {
    if (!out4) throw ApiError{MRT_ERR_INVALID, "null output"};
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out4, c->dbg.p, 16, hipMemcpyDeviceToHost));
  });
}

int mrt_debug_build(void) {
#ifdef MRT_DEBUG_BOUNDS
  return 1;
#else
  return 0;
#endif
}

int mrt_shard_pixels(uint32_t W, uint32_t H, uint32_t si, uint32_t sc, uint32_t* pixels, uint32_t* count) {
  try {
    if (!count) throw ApiError{MRT_ERR_INVALID, "null count"};
    check_image_size(W, H);
    if (sc == 0) sc = 1;
    if (si >= sc) throw ApiError{MRT_ERR_INVALID, "shard_index >= shard_count"};
    const std::vector<uint32_t> list = shard_pixel_list(W, H, si, sc);
    *count = (uint32_t)list.size();
    if (pixels && !list.empty()) memcpy(pixels, list.data(), list.size() * 4);
    return MRT_OK;
  } catch (const ApiError& e) {
    mrt_global_error = e.msg;
    return e.code;
  } catch (const std::bad_alloc&) {
    mrt_global_error = "out of host memory";
    return MRT_ERR_NOMEM;
  }
}

}  // extern "C"
