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
  if (id == OPT_QUEUES && v != c->opt[id] && c->pool_mem) {  // the pool is split per queue: reallocated at the next render
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
      HIP_CHECK(hipMalloc(&q.ctrl, sizeof(Ctrl)));
      HIP_CHECK(hipHostMalloc(&q.h_stat, 2 * sizeof(HostStatus), hipHostMallocCoherent | hipHostMallocMapped));
      memset(q.h_stat, 0, 2 * sizeof(HostStatus));
      HIP_CHECK(hipHostGetDevicePointer((void**)&q.d_stat, q.h_stat, 0));
      HIP_CHECK(hipEventCreateWithFlags(&q.ev[0], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&q.ev[1], hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&q.join, hipEventDisableTiming));
    }
    HIP_CHECK(hipMalloc(&c->work, 256));
    HIP_CHECK(hipMemset(c->work, 0, 256));
    HIP_CHECK(hipEventCreateWithFlags(&c->acc_done, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&c->set_fork, hipEventDisableTiming));
    HIP_CHECK(hipMalloc(&c->d_cnt, sizeof(DevCounters)));
    HIP_CHECK(hipMemset(c->d_cnt, 0, sizeof(DevCounters)));
    HIP_CHECK(hipMalloc(&c->dbg, 16));
    HIP_CHECK(hipMemset(c->dbg, 0, 16));
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
  hipFree(c->scene_mem);
  hipFree(c->pool_mem);
  hipFree(c->results);
  if (c->acc_done) hipEventDestroy(c->acc_done);
  if (c->set_fork) hipEventDestroy(c->set_fork);
  hipFree(c->work);
  hipFree(c->gamma_d);
  for (Queue& q : c->q) {
    hipFree(q.ctrl);
    if (q.h_stat) hipHostFree(q.h_stat);
    for (hipEvent_t e : {q.ev[0], q.ev[1], q.join})
      if (e) hipEventDestroy(e);
    if (q.stream) hipStreamDestroy(q.stream);
  }
  hipFree(c->d_cnt);
  hipFree(c->dbg);
  hipFree(c->d_acc_rgb);
  hipFree(c->d_acc_b);
  hipFree(c->d_rays);
  hipFree(c->d_rhits);
  hipFree(c->dn_mem);
  hipFree(c->slot_ro);
  for (auto& kv : c->pixlists) hipFree(kv.second.first);
  if (c->tev[0]) hipEventDestroy(c->tev[0]);
  if (c->tev[1]) hipEventDestroy(c->tev[1]);
  for (hipEvent_t e : c->ev_pool) hipEventDestroy(e);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
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
    // one allocation, 256-B aligned sections
    size_t off = 0;
    auto sec = [&](size_t bytes) {
      size_t o = off;
      off += (bytes + 255) & ~(size_t)255;
      return o;
    };
    size_t o_slots = sec(hs.slots.size() * 4), o_stl = sec(hs.slots_tl.size() * 4), o_tlet = sec(hs.tlet.size() * 4),
           o_inv = sec(hs.inst_inv.size() * 4),
           o_fwd = sec(hs.inst_fwd.size() * 4), o_imat = sec(hs.inst_mat.size() * 4),
           o_mmat = sec(hs.model_mat.size() * 4), o_sph = sec(hs.sph.size() * 4), o_smat = sec(hs.sph_mat.size() * 4),
           o_tri = sec(hs.tri_shade.size() * 4), o_mat = sec(hs.materials.size() * sizeof(GpuMaterial)),
           o_tex = sec(hs.textures.size() * sizeof(GpuTexture)), o_texel = sec(hs.texels.size() * 4),
           o_vnid = sec(hs.vol_nid.size() * 4), o_vmat = sec(hs.vol_mat.size() * 4);
    const std::vector<float>& ln_table = hs.ln_table;
    const size_t o_ln = sec(ln_table.size() * 4);
    const size_t o_sops = sec(hs.surf_ops.size() * sizeof(GpuSurfOp));
    const size_t o_bgf = sec(hs.bg_faces.size() * sizeof(GpuSurfRef));
    const size_t o_bgm = sec(sizeof(hs.bg_m));
    const size_t o_vnf = sec(hs.vnf_leaf.size() * 4);
    const size_t o_eve = sec(hs.eve.size() * 4), o_tb = sec(hs.tri_tb.size() * 4);
    if (c->scene_mem) HIP_CHECK(hipFree(c->scene_mem));
    c->scene_mem = nullptr;
    c->has_scene = false;
    HIP_CHECK(hipMalloc(&c->scene_mem, off + 256));
    char* base = (char*)c->scene_mem;
    auto up = [&](size_t o, const void* src, size_t bytes) {
      if (bytes) HIP_CHECK(hipMemcpy(base + o, src, bytes, hipMemcpyHostToDevice));
    };
    up(o_slots, hs.slots.data(), hs.slots.size() * 4);
    up(o_stl, hs.slots_tl.data(), hs.slots_tl.size() * 4);
    up(o_tlet, hs.tlet.data(), hs.tlet.size() * 4);
    up(o_vnid, hs.vol_nid.data(), hs.vol_nid.size() * 4);
    up(o_vmat, hs.vol_mat.data(), hs.vol_mat.size() * 4);
    up(o_ln, ln_table.data(), ln_table.size() * 4);
    up(o_inv, hs.inst_inv.data(), hs.inst_inv.size() * 4);
    up(o_fwd, hs.inst_fwd.data(), hs.inst_fwd.size() * 4);
    up(o_imat, hs.inst_mat.data(), hs.inst_mat.size() * 4);
    up(o_mmat, hs.model_mat.data(), hs.model_mat.size() * 4);
    up(o_sph, hs.sph.data(), hs.sph.size() * 4);
    up(o_smat, hs.sph_mat.data(), hs.sph_mat.size() * 4);
    up(o_tri, hs.tri_shade.data(), hs.tri_shade.size() * 4);
    up(o_mat, hs.materials.data(), hs.materials.size() * sizeof(GpuMaterial));
    up(o_tex, hs.textures.data(), hs.textures.size() * sizeof(GpuTexture));
    up(o_texel, hs.texels.data(), hs.texels.size() * 4);
    up(o_sops, hs.surf_ops.data(), hs.surf_ops.size() * sizeof(GpuSurfOp));
    up(o_bgf, hs.bg_faces.data(), hs.bg_faces.size() * sizeof(GpuSurfRef));
    up(o_bgm, hs.bg_m, sizeof(hs.bg_m));
    up(o_vnf, hs.vnf_leaf.data(), hs.vnf_leaf.size() * 4);
    up(o_eve, hs.eve.data(), hs.eve.size() * 4);
    up(o_tb, hs.tri_tb.data(), hs.tri_tb.size() * 4);
    DevScene S = host_dev_scene(hs);  // sizes and flags; its pointers now go to the device copies
    S.slots = (const uint32_t*)(base + o_slots);
    S.slots_tl = (const uint32_t*)(base + o_stl);
    S.tlet = (const uint32_t*)(base + o_tlet);
    S.n_tlet = (uint32_t)(hs.tlet.size() / 4);
    S.tl_world_begin = hs.tl_world_begin;
    S.inst_inv = (const float*)(base + o_inv);
    S.inst_fwd = (const float*)(base + o_fwd);
    S.inst_mat = (const uint32_t*)(base + o_imat);
    S.model_mat = (const uint32_t*)(base + o_mmat);
    S.sph = (const float*)(base + o_sph);
    S.sph_mat = (const uint32_t*)(base + o_smat);
    S.tri_shade = (const float*)(base + o_tri);
    S.materials = (const GpuMaterial*)(base + o_mat);
    S.textures = (const GpuTexture*)(base + o_tex);
    S.texels = (const uint32_t*)(base + o_texel);
    S.vol_nid = (const float*)(base + o_vnid);
    S.vol_mat = (const uint32_t*)(base + o_vmat);
    S.ln_table = ln_table.empty() ? nullptr : (const float*)(base + o_ln);
    S.dbg = c->dbg;
    S.surf_ops = (const GpuSurfOp*)(base + o_sops);
    S.bg_faces = (const GpuSurfRef*)(base + o_bgf);
    S.bg_m = (const float*)(base + o_bgm);
    S.vnf_leaf = (const uint32_t*)(base + o_vnf);
    S.eve = (const float*)(base + o_eve);
    S.tri_tb = hs.tri_tb.empty() ? nullptr : (const float*)(base + o_tb);
    c->S = S;
    c->scene_bytes = off;
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
    DevCamera d;
    d.origin = V3{cam->origin[0], cam->origin[1], cam->origin[2]};
    d.llc = V3{cam->lower_left_corner[0], cam->lower_left_corner[1], cam->lower_left_corner[2]};
    d.horizontal = V3{cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]};
    d.vertical = V3{cam->vertical[0], cam->vertical[1], cam->vertical[2]};
    d.u = V3{cam->u[0], cam->u[1], cam->u[2]};
    d.v = V3{cam->v[0], cam->v[1], cam->v[2]};
    d.lens_radius = cam->lens_radius;
    c->cam = d;
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
    HIP_CHECK(hipMemcpy(&h, c->d_cnt, sizeof(h), hipMemcpyDeviceToHost));
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
    HIP_CHECK(hipMemset(c->d_cnt, 0, sizeof(DevCounters)));
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
    HIP_CHECK(hipMemcpy(out4, c->dbg, 16, hipMemcpyDeviceToHost));
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
    if (W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 32)) throw ApiError{MRT_ERR_INVALID, "bad image size"};
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
