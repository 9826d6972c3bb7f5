// ctx.h — the single-device context behind the C ABI (include/massrt.h) and
// the host functions that trace.hip, render.hip, passes.hip and api.hip
// share. Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <atomic>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../../include/massrt.h"
#include "../host/adaptive.h"
#include "../host/loop.h"
#include "../host/options.h"
#include "devmem.h"
#include "frames.h"
#include "pool.h"

struct HipError {
  std::string msg;
};
#define HIP_CHECK(x)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) throw HipError{std::string(#x) + ": " + hipGetErrorString(e_)}; \
  } while (0)

struct ApiError {
  int code;
  std::string msg;
};

inline void check_image_size(uint32_t W, uint32_t H) {
  if (W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 32)) throw ApiError{MRT_ERR_INVALID, "bad image size"};
}

// One independent path pool driven on its own stream. Several queues share
// the work counter and run concurrently, so one queue's k_trace tail (the
// last long rays on few lanes) overlaps the other queues' kernels instead of
// idling the GPU.
struct Queue {
  hipStream_t stream = nullptr;
  PathBufs bufs[2]{};   // views into the context's pool, as is hits
  uint4* hits = nullptr;
  size_t cap = 0;       // paths
  DevBuf<Ctrl> ctrl;
  HostStatus* h_stat = nullptr;  // pinned coherent, 2 slots, written by k_status (lagged status reads)
  HostStatus* d_stat = nullptr;  // the same memory as the device addresses it
  hipEvent_t ev[2]{};
  hipEvent_t join = nullptr;
};

// A round's word of mrt_render_adaptive: the pixels and the tiles still open
// after its evaluation, the next round's list length among them.
struct AdaptWord {
  uint32_t pixels, tiles;
};

struct mrt_ctx {
  int device = 0;
  MultiDev* multi = nullptr;  // a context over several devices (frames.hip): the rest is unused
  std::atomic<int> images{0};  // live mrt_image objects created on this handle (any thread)
  hipStream_t stream = nullptr;
  std::string err;
  // scene
  DevBuf<char> scene;      // every array of S, one allocation (upload.h plan_scene)
  size_t scene_bytes = 0;  // the sections alone (mrt_scene_device_bytes)
  mrt::DevScene S{};
  bool has_scene = false;
  mrt::DevCamera cam{};
  bool has_camera = false;
  // options: the values set (mrt_set_option; kOptDefs), what the rules know
  // about the scene, and everything derived from the two (apply_options)
  int64_t opt[mrt::kNumOpts];
  mrt::SceneFacts facts;
  mrt::Tuning tun{};
  bool scene_alpha = true;  // the scene has alpha-tested triangles
  bool scene_vblas = false;  // a volume whose target is an instance or a model (k_trace's VBLAS variants)
  bool scene_ext = false;   // composite surfaces, a CubeMap background or Eve materials (the EXT kernel variants)
  // render state
  size_t pool_cap = 0;  // paths over all queues
  DevBuf<char> pool;
  Queue q[mrt::kMaxQueues];
  DevBuf<uint32_t> work;     // shared work counter of the wavefront loop (word 1: tonemap max count)
  DevBuf<uint32_t> gamma_d;  // display: gamma byte thresholds (256 words)
  DevBuf<float4> results;    // the results slab, one float4 per sample
  // acc_done: recorded on the caller's stream after the accumulate that read
  // the results slab (and after any other caller-stream work on the shared
  // buffers, mark_ctx_busy); the next render's queues fork after it.
  // (Round 2's two alternating queue sets, measured 5-12% slower, are in
  // profiles/r3_experiments/ab_branches.patch.)
  hipEvent_t acc_done = nullptr;
  hipEvent_t set_fork = nullptr;
  // kernel-timing marks resolved lazily (mrt_get_kernel_stats): a timed
  // render does not wait for its set's drain
  std::vector<std::array<hipEvent_t, 3>> pend_marks;
  std::vector<std::array<hipEvent_t, 2>> pend_fin;
  DevBuf<mrt::DevCounters> d_cnt;
  DevBuf<uint32_t> dbg;  // MRT_DEBUG_BOUNDS record (4 words)
  int cus = 1;
  uint32_t trace_grid = 1024;   // k_trace_simple workgroups (cus * 4)
  uint32_t refill_grid = 2048;  // k_refill workgroups (grid-stride; cus * 8)
  std::map<std::pair<const void*, size_t>, uint32_t> grids;  // persistent grid per (kernel, LDS bytes)
  // k_render: per-lane current world ray, origins then directions in one
  // buffer (ensure_slots sets the two views); event pair timing one launch
  DevBuf<float4> slots;
  float4* slot_ro = nullptr;
  float4* slot_rd = nullptr;
  hipEvent_t tev[2] = {nullptr, nullptr};

  // pixel lists by (W, H, shard_index, shard_count, n_views); n_views 0: one frame's list
  std::map<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t, uint32_t>, DevBuf<uint32_t>> pixlists;
  DevBuf<DevView> views;  // the view table of the last mrt_render_views (grown on demand; the kernels only read it)
  std::vector<DevView> views_h;  // its host copy, the upload's source
  // mrt_render_rays: the identity list its accumulate takes (grown on demand, filled once on the stream of the call
  // that grew it: ids_ready, which every call's stream waits for), the host form's copy of the caller's table, and
  // the event that orders the queues after the caller's stream, the table's writer
  DevBuf<uint32_t> ray_ids;
  hipEvent_t ids_ready = nullptr;
  DevBuf<mrt_path_ray> rays_d;
  hipEvent_t rays_ready = nullptr;
  // mrt_render_adaptive: a byte per shard tile (1: still in the running), the scan's words (an offset per tile, then
  // {pixels, open tiles} per kBlock tiles), the next round's pixel list (two, alternating), and one word per round
  // that k_adaptive_scan_blocks writes into pinned host memory and the host reads behind ad_ev. All grown on demand
  // (adaptive_scratch); a call returns only when its kernels have ended, so between calls nothing reads them
  DevBuf<uint8_t> ad_open;
  DevBuf<uint32_t> ad_scan;
  DevBuf<uint32_t> ad_list[2];
  AdaptWord* ad_words_h = nullptr;  // pinned coherent, kAdaptMaxRounds words
  AdaptWord* ad_words_d = nullptr;  // the same memory as the device addresses it
  hipEvent_t ad_ev = nullptr;
  // host-buffer render staging
  DevBuf<float> d_acc_rgb;
  DevBuf<uint32_t> d_acc_b;
  DevBuf<float> d_acc_mom;     // mrt_render_adaptive's moments and counts
  DevBuf<uint32_t> d_acc_n;
  // kernel timing
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  mrt_kernel_stats kstats{};
  // device ray buffer for mrt_trace_rays
  DevBuf<float> d_rays;
  DevBuf<uint4> d_rhits;
  // denoise.hip scratch: colour A, colour B (one float4 per pixel each), guides (two float4 per pixel)
  DevBuf<float4> dn_mem;
};

// errors without a context (api.hip); not exported from the library
__attribute__((visibility("hidden"))) extern thread_local std::string mrt_global_error;

// Runs f on the context's device; exceptions become the context's error text
// and an MRT_ERR_* code.
template <typename F>
int guarded(mrt_ctx* c, F&& f) {
  if (!c) {
    mrt_global_error = "null context";
    return MRT_ERR_INVALID;
  }
  try {
    HIP_CHECK(hipSetDevice(c->device));
    f();
    c->err.clear();
    return MRT_OK;
  } catch (const ApiError& e) {
    c->err = e.msg;
    return e.code;
  } catch (const HipError& e) {
    c->err = e.msg;
    return MRT_ERR_HIP;
  } catch (const std::bad_alloc&) {
    c->err = "out of host memory";
    return MRT_ERR_NOMEM;
  } catch (const std::exception& e) {
    c->err = e.what();
    return MRT_ERR_INVALID;
  }
}

// A multi-device handle (mrt_create_multi): entry points that act on one
// device run on device 0; scene and camera go to every device.
template <typename F>
int on_dev0(mrt_ctx* c, F&& f) {
  mrt_ctx* d = multi_dev(c->multi, 0);
  const int rc = f(d);
  c->err = d->err;
  return rc;
}
template <typename F>
int on_each(mrt_ctx* c, F&& f) {
  for (int i = 0; i < multi_count(c->multi); ++i) {
    mrt_ctx* d = multi_dev(c->multi, i);
    const int rc = f(d);
    if (rc != MRT_OK) {
      c->err = d->err;
      return rc;
    }
  }
  c->err.clear();
  return MRT_OK;
}
#define MRT_DEV0(c, call) \
  if ((c) && (c)->multi) return on_dev0((c), [&](mrt_ctx* c) { return call; })
#define MRT_EACH(c, call) \
  if ((c) && (c)->multi) return on_each((c), [&](mrt_ctx* c) { return call; })

// A runtime value as a template argument, for choosing among a kernel's
// variants: f(std::integral_constant<V>) for the first of V, Vs... that equals
// v, for the last if none does.
template <auto V, auto... Vs, typename T, typename F>
auto with_value(T v, F&& f) {
  if constexpr (sizeof...(Vs) == 0)
    return f(std::integral_constant<decltype(V), V>{});
  else
    return v == V ? f(std::integral_constant<decltype(V), V>{}) : with_value<Vs...>(v, f);
}

// ---- trace.hip ----
// k_trace over pool buffer `in` of queue `q`, specialised on the scene, on stream `st`
void launch_trace(mrt_ctx* c, hipStream_t st, const Queue& q, const PathBufs& in, uint32_t cur, bool count,
                  float tmin, float tmax);
void launch_trace_simple(mrt_ctx* c, const Queue& q, uint32_t cur);  // MRT_RENDER_SIMPLE_TRACE, on the queue's stream
uint32_t persistent_grid(mrt_ctx* c, const void* f, size_t smem, bool shared = false, int block = kBlock,
                         int share_num = 3, int share_den = 4);

// ---- render.hip ----
void wait_queues(mrt_ctx* c, hipStream_t st);
void release_pool(mrt_ctx* c);  // frees the path pool; the caller has synchronised the device
void ensure_pool(mrt_ctx* c, size_t P);
void ensure_slots(mrt_ctx* c, size_t n);
std::vector<uint32_t> shard_pixel_list(uint32_t W, uint32_t H, uint32_t si, uint32_t sc);
std::pair<uint32_t*, uint32_t> pixlist(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc,
                                       uint32_t n_views = 0);
void mark_ctx_busy(mrt_ctx* c, hipStream_t st);
mrt::DevCamera dev_camera(const mrt_camera& cam);
void resolve_kernel_timing(mrt_ctx* c);

// ---- adaptive.hip ----
// k_accumulate with the moments and counts of mrt_render_adaptive beside the sums (render_wavefront's other accumulate)
void accumulate_moments(mrt_ctx* c, const RenderParams& rp, float* d_rgb, uint32_t* d_b, float* d_moments,
                        uint32_t* d_samples, hipStream_t st);
mrt::AdaptFrame adaptive_frame(mrt_ctx* c, uint32_t W, uint32_t H, uint32_t si, uint32_t sc);  // checked
void adaptive_scratch(mrt_ctx* c, uint32_t n_tiles, uint32_t n_pix);
void adaptive_evaluate(const mrt::AdaptFrame& f, const float* d_moments, const uint32_t* d_samples, float tau2,
                       float floor, uint8_t* d_open, bool only_running, uint32_t* d_n_open, hipStream_t st);
AdaptWord adaptive_compact(mrt_ctx* c, const mrt::AdaptFrame& f, uint32_t* list, uint32_t list_cap, uint32_t round,
                           hipStream_t st);
