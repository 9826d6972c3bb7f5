// slab_check — k_trace's two walks run on the host, no GPU needed: a driver of
// the device headers' own step functions (walk.h trav_*, walk_nf.h trav_*_nf /
// nf_finish, compiled here for the host: the same source, the same bits) over
// the record stream of a built-in scene, on camera rays, one-bounce rays and
// stress rays. What is written here is only the evidence that must stay
// independent of that code:
//   * box_exact, BoundingBox::hit with IEEE quotients (geom.rs:218-247): every
//     box the early slab decision settles, and every answer of the exact test
//     (box_hit_exact, the qfast path), must equal it; the fraction left to the
//     exact test is reported. Round 2 used it to find that mesh_ply's vertices
//     at ~1e-16 (sin(pi)) had switched the whole scene to the exact test.
//   * the double-precision bound checks (check_hit, check_hit_wild,
//     cone_rho_min): every hit the reference's tests accept lies within the
//     near-first walk's rounding margin of its boxes (nf_bound.h).
//   * the comparison of the two walks' closest hits, the sibling layout
//     against the plain preorder stream, and the walk statistics.
//   hipcc --offload-host-only -x hip -O2 -std=c++17 -ffp-contract=off -fno-fast-math -o tools/slab_check
//       tools/slab_check.cpp -Lmass-raytrace_amd/massrt -lmassrt -Wl,-rpath,$PWD/mass-raytrace_amd/massrt
//   (plain g++ -O2 -std=c++17 -ffp-contract=off builds it too, to the same output: devbase.h's fallback types)
//   tools/slab_check mesh_ply 20000 assets [layout | nf | graze | tangent]
//   tools/slab_check cornell 0 tests/golden hits|hits-nf rays.f32 out.u32
//       n x 6 float32 rays in, n x 4 uint32 out in mrt_trace_rays' layout (k_rays_in -> walk -> k_rays_out)
//   tools/slab_check eve 0 assets stream
//       element counts and hashes of the stream, its tables and the treelet (stream_mode)
//   tools/slab_check @world.txt 0 - hits|hits-nf rays.f32 out.u32 [starts.u8]
//       the scene is the world file's (load_world below; tests/adversarial_worlds.py writes them), built with the
//       seed the file names; prints the walk's fallbacks and how many rays started on the reference walk, and
//       with one more path writes a byte per ray: 1, the ray started near first
//   tools/slab_check @world.txt 0 - bound rays.f32
//       the double-precision bound checks on the file's rays (the `nf bound:` line)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <unordered_map>
#include <vector>

#include "../mass-raytrace_amd/csrc/device/material.h"
#include "../mass-raytrace_amd/csrc/device/records.h"
#include "../mass-raytrace_amd/csrc/device/upload.h"
#include "../mass-raytrace_amd/csrc/device/walk_nf.h"

using namespace mrt;

namespace {

using V = V3;
const float kTmin = 0.001f;

// BoundingBox::hit with IEEE quotients (fminf/fmaxf = minNum/maxNum, as v_min/v_max)
bool box_exact(V mn, V mx, V o, V d, float tmin, float tmax) {
  const float lo[3] = {mn.x, mn.y, mn.z}, hi[3] = {mx.x, mx.y, mx.z}, oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
  float a[3], b[3];
  for (int k = 0; k < 3; ++k) a[k] = (lo[k] - oo[k]) / dd[k], b[k] = (hi[k] - oo[k]) / dd[k];
  const float t0 = fmaxf(fmaxf(fminf(a[0], b[0]), fminf(a[1], b[1])), fmaxf(fminf(a[2], b[2]), tmin));
  const float t1 = fminf(fminf(fmaxf(a[0], b[0]), fmaxf(a[1], b[1])), fminf(fmaxf(a[2], b[2]), tmax));
  return !(t1 < t0);
}

struct Stats {
  uint64_t boxes = 0, undecided = 0, wrong = 0;
  uint64_t loads = 0;  // 16-B record loads (k_trace's vector-memory instructions per lane step)
  uint64_t entries = 0;  // instance entries (each: a transform, the object margin, the world ray back)
  uint64_t wild_skips = 0;  // wild instances passed by on their own box test
  uint64_t prims = 0;       // primitive tests
};

// `bound` checks (nf_bound.h): every primitive test of the
// reference walk is repeated with t_max = inf; an accepted hit X = o + t d
// (exact, in double) must lie within rho(L = t |d|) of the primitive's NF leaf
// box in its own space, and an instance's hit within the world rho of the
// instance's world box (unless it is wild: never culled)
struct BoundCheck {
  uint64_t checks = 0, outside = 0, over = 0, wild_checks = 0;
  double worst = 0, worst_cap = 0, worst_wild = 0;  // max dist / rho, max L / L_cap, the wild margin's max dist / rho
};
BoundCheck* g_bc = nullptr;
// instance id -> its WILD entry's first slot (nf_bound.h NfWild; 0: not wild)
std::unordered_map<uint32_t, uint32_t> g_wild_entry;
NfWild wild_entry(const HostScene& s, uint32_t at) { return rec::nf_wild_entry(s.slots.data(), at); }

// NF tree parents (normal cones, round 6): every node a primitive's test
// passes through on the near-first walk thickens its boxes by that node's
// rho, so each must cover the hit: leaf_parent[vnf slot] is the NF node
// holding the primitive's leaf, nf_parent the node above a node (~0: a root)
std::unordered_map<uint32_t, uint32_t> g_nf_parent;
std::vector<uint32_t> g_leaf_parent;
void map_nf_tree(const HostScene& s, uint32_t root, std::vector<uint8_t>& seen_blas) {
  const uint32_t* w = s.slots.data();
  std::vector<std::pair<uint32_t, uint32_t>> st{{root, ~0u}};
  while (!st.empty()) {
    const auto [i, par] = st.back();
    st.pop_back();
    if (rec::is_box(w, i)) {
      g_nf_parent[i] = par;
      const uint32_t base = rec::nf_children(w, i);
      st.push_back({base, i});
      st.push_back({base + rec::nf_left_slots(w, i), i});
      continue;
    }
    for (uint32_t r = i; r != kNfPop; r = rec::nf_next(w, r)) {  // the leaf's records
      g_leaf_parent[rec::vnf_slot(w, r, s.vnf_base)] = par;
      const uint32_t k = rec::kind(w, r);
      if (k != KIND_INST && k != KIND_MODEL) continue;
      if (k == KIND_INST && rec::nf_wild(w, r) != 0) g_wild_entry[rec::object_id(w, r)] = rec::nf_wild(w, r);
      const uint32_t blas = rec::nf_blas_root(w, r);
      if (!seen_blas[blas]) {
        seen_blas[blas] = 1;
        map_nf_tree(s, blas, seen_blas);
      }
    }
  }
}
// the smallest rho over the NF nodes a hit's primitive (vnf slot) sits below,
// each with its normal cone (walk_nf.h trav_box_index_nf), at the hit's t
float cone_rho_min(const HostScene& s, uint32_t vslot, V o, V d, float t, bool obj) {
  const float d2 = (d.x * d.x + d.y * d.y) + d.z * d.z;
  const NfBound& B = s.nfb;
  const NfCoef c = obj ? nf_coef_object(B, o, d2) : nf_coef_world(B, o, d2);
  const NfLine l = nf_line(B, c, t, obj ? B.ao0 : B.aw0, obj ? B.ao1 : B.aw1, d2, d);
  float rho = nf_rho_at(B, c, t);
  if (!(B.kc > 0) || vslot >= g_leaf_parent.size()) return rho;
  const uint32_t* w = s.slots.data();
  for (uint32_t n = g_leaf_parent[vslot]; n != ~0u; n = g_nf_parent[n]) {
    const rec::NfFrame a = rec::nf_frame(w, n);
    rho = std::min(rho, nf_rho_cone(l, t, a.ox, a.oy, a.oz, a.ew, d));
  }
  return rho;
}
double box_dist(const float* b, double x, double y, double z) {
  const double p[3] = {x, y, z};
  double m = 0;
  for (int k = 0; k < 3; ++k) m = std::max(m, std::max((double)b[k] - p[k], p[k] - (double)b[3 + k]));
  return m;
}
void check_hit(const HostScene& s, const float* box, V o, V d, float t, bool obj, uint32_t vslot = ~0u) {
  if (!box || std::isnan(box[0])) return;
  const double x = (double)o.x + (double)t * d.x, y = (double)o.y + (double)t * d.y, z = (double)o.z + (double)t * d.z;
  const NfCoef c = obj ? nf_coef_object(s.nfb, o, dot(d, d)) : nf_coef_world(s.nfb, o, dot(d, d));
  // the rho of every NF node above the primitive, narrowed by its cone
  const float rho = vslot == ~0u ? nf_rho_at(s.nfb, c, t) : cone_rho_min(s, vslot, o, d, t, obj);
  const float cap = nf_rho_at(s.nfb, c, INFINITY);
  const double dist = box_dist(box, x, y, z);

  g_bc->checks++;
  if (dist > 0) g_bc->outside++;
  const double ratio = dist / (double)rho;
  if (ratio > 1) {
    if (g_bc->over < 5)
      fprintf(stderr, "bound exceeded: dist %.3e rho %.3e (%s space) t %a\n", dist, (double)rho, obj ? "object" : "world", t);
    g_bc->over++;
  }
  g_bc->worst = std::max(g_bc->worst, ratio);
  // the cap: rho at the capped L must still cover this hit
  if (dist > cap) g_bc->over++;
}
// a wild instance's hit in world space against its world box, within the wild margin
void check_hit_wild(const HostScene& s, uint32_t inst, V o, V d, float t) {
  auto it = g_wild_entry.find(inst);
  if (it == g_wild_entry.end()) return;  // no entry (an infinite box): always entered
  const NfWild e = wild_entry(s, it->second);
  const float box[6] = {e.mn[0], e.mn[1], e.mn[2], e.mx[0], e.mx[1], e.mx[2]};
  const double x = (double)o.x + (double)t * d.x, y = (double)o.y + (double)t * d.y, z = (double)o.z + (double)t * d.z;
  const float rho = nf_rho_wild(e, o, dot(d, d), t), cap = nf_rho_wild(e, o, dot(d, d), INFINITY);
  const double dist = box_dist(box, x, y, z);
  g_bc->checks++;
  g_bc->wild_checks++;
  if (dist > 0) g_bc->outside++;
  const double ratio = dist / (double)rho;
  if (ratio > 1 || dist > cap) {
    if (g_bc->over < 5) fprintf(stderr, "wild bound exceeded: dist %.3e rho %.3e t %a\n", dist, (double)rho, t);
    g_bc->over++;
  }
  g_bc->worst = std::max(g_bc->worst, ratio);
  g_bc->worst_wild = std::max(g_bc->worst_wild, ratio);
}
const float* leaf_box(const HostScene& s, uint32_t base, uint32_t id) {
  if (s.nf_leaf_box.empty()) return nullptr;
  return &s.nf_leaf_box[6 * (size_t)(s.vnf_base[base] + id)];
}

// ---- the driver: one ray at a time through the device headers' steps ----------
// A one-ray pool (k_rays_in's slot 0) and the walk's inputs over it.
struct OneRay {
  float4 ro, rd;
  TravIn in;
  OneRay(const DevScene& S, V o, V d)
      : ro(make_float4(o.x, o.y, o.z, 0.0f)), rd(make_float4(d.x, d.y, d.z, 0.0f)),
        in{S, reinterpret_cast<const uint4*>(S.slots), S.world_begin, &ro, &rd, kTmin} {}
};
struct Scene {
  const HostScene& s;
  DevScene S;
  explicit Scene(const HostScene& hs) : s(hs), S(host_dev_scene(hs)) {}
};
V box_lo(const Trav& t) { return V{u2f(t.s0.x), u2f(t.s0.y), u2f(t.s0.z)}; }
V box_hi(const Trav& t) { return V{u2f(t.s0.w), u2f(t.s1.x), u2f(t.s1.y)}; }

// Before a reference box step: the early slab decision (slab_fast /
// slab_margin, where it decides) and the exact test (box_hit_exact: qfast in
// its domain) against the IEEE-quotient truth.
void check_box(const TravIn& in, const Trav& t, Stats& st) {
  const V mn = box_lo(t), mx = box_hi(t);
  const bool truth = box_exact(mn, mx, t.r.o, t.r.d, in.tmin, t.best);
  float t0, t1;
  slab_fast(mn, mx, t.r, in.tmin, t.best, t0, t1);
  const float m = slab_margin(t.r, t0, t1), gap = t1 - t0;
  if (gap > m) st.wrong += !truth;
  else if (-gap > m) st.wrong += truth;
  st.wrong += box_hit_exact(mn, mx, t.r, in.tmin, t.best) != truth;
}
// Before a reference primitive step: the bound checks of its record, the real
// test repeated at t_max = inf ((wo, wd): the world ray)
void check_prim(const HostScene& s, const TravIn& in, const Trav& t, V wo, V wd) {
  const uint4 s0 = t.s0, s1 = t.s1;
  float th;
  if (s1.w == KIND_SPHERE) {  // spheres are world objects
    if (sphere_hit(V{u2f(s0.x), u2f(s0.y), u2f(s0.z)}, u2f(s0.w), t.r.o, t.r.d, t.r.a, in.tmin, INFINITY, th))
      check_hit(s, leaf_box(s, VNF_SPHERE, s1.x), t.r.o, t.r.d, th, false);
  } else if (s1.w == KIND_TRI) {
    const uint4 s2 = rec_load1<false>(in, t.i + 2);
    const V a{u2f(s0.x), u2f(s0.y), u2f(s0.z)}, ab{u2f(s0.w), u2f(s1.x), u2f(s1.y)}, ac{u2f(s2.x), u2f(s2.y), u2f(s2.z)};
    if (!tri_hit(a, ab, ac, t.r.o, t.r.d, in.tmin, INFINITY, th)) return;
    const uint32_t id = s1.z & kTriIdMask;
    const bool inst = t.ret != kNoRet && (t.ret & kRetInstance);
    check_hit(s, leaf_box(s, VNF_TRI, id), t.r.o, t.r.d, th, inst, s.vnf_base[VNF_TRI] + id);
    if (t.ret == kNoRet) return;
    // the same hit in world space against the container's world box
    const uint32_t cid = rec_load1<false>(in, (t.ret & ~kRetInstance) - 2).x;
    if (!inst) check_hit(s, leaf_box(s, VNF_MODEL, cid), wo, wd, th, false);
    else if (s.nf_inst_wild.empty() || !s.nf_inst_wild[cid]) check_hit(s, leaf_box(s, VNF_INST, cid), wo, wd, th, false);
    else check_hit_wild(s, cid, wo, wd, th);  // its world box within the wild margin (nf_bound.h nf_rho_wild)
  }
}

// One step of the reference walk and the fetch of the next record, through
// k_trace's own dispatch (walk_nf.h trav_*_either; NF, WILD: the kernel's
// variant). st: the record loads of the step by kind; check: the box and
// bound checks too.
template <uint32_t ALPHA, bool NF = false, bool WILD = false>
void ref_step(const Scene& c, const TravIn& in, const NfStack& stk, Trav& t, LocalCounters& lc, Stats* st, bool check,
              V wo, V wd) {
  if (trav_at_box(t)) {
    if (st) st->loads += 2;
    if (st && check) check_box(in, t, *st);
    trav_box_index_either<true, NF, WILD>(in, stk, t, lc);
  } else {
    const uint32_t kind = t.s1.w;
    if (st) st->loads += kind == KIND_TRI ? 3 : kind == KIND_INST ? 5 : 2;  // END, sphere, model: 2
    if (st && kind == KIND_INST) st->entries++;
    if (check && g_bc) check_prim(c.s, in, t, wo, wd);
    trav_prim_index_either<true, ALPHA, false, false, false, NF, WILD>(in, stk, t, lc);
  }
  if (trav_may_fetch<NF, WILD>(t)) trav_fetch(in, t);
}

// The reference's walk (k_trace's exact variant, one lane).
template <uint32_t ALPHA>
Hit walk_ref(const Scene& c, V o, V d, Stats* st = nullptr, bool check = false) {
  OneRay p(c.S, o, d);
  Trav t;
  LocalCounters lc;
  trav_init(p.in, t, 0, INFINITY);
  while (!t.done) ref_step<ALPHA>(c, p.in, NfStack{nullptr, 0}, t, lc, st, check, o, d);  // no stack: NF = false
  if (st) st->boxes += lc.node_visits, st->undecided += lc.box_exact;
  return trav_hit(p.in, t);
}

// The verified near-first walk in the per-lane order of k_trace's NF variant:
// the reference's steps once it has fallen back, the winner's check when the
// walk is over, else a near-first step.
// WILD: the scene has a wild tree (k_trace's variant for it, trace.hip launch_trace)
template <uint32_t ALPHA, bool WILD>
Hit walk_nf_w(const Scene& c, V o, V d, Stats& st, uint64_t& fallbacks, uint64_t& starts_ref) {
  OneRay p(c.S, o, d);
  const TravIn& in = p.in;
  // two words beyond kNfStack: a step pushes at most two, so an overflow is
  // seen after the step that made it instead of being written out of bounds
  uint32_t words[kNfStack + 2];
  const NfStack stk{words, 1};
  Trav t;
  LocalCounters lc;
  trav_init_nf<WILD>(in, stk, t, 0, INFINITY, c.S.nf_world);  // as k_trace: with a wild tree its marker goes to the stack first
  if (t.sp == kExactMode) ++starts_ref;  // nf_start: the bound does not cover this ray
  while (!t.done) {
    if (t.sp == kExactMode) {
      ref_step<ALPHA, true, WILD>(c, in, stk, t, lc, &st, false, o, d);
      continue;
    }
    if (WILD && t.sp == kNfWait) {  // k_trace sends a batch of such lanes into the wild tree; one lane is its own batch
      nf_resume_wild(in, t);
      trav_fetch(in, t);
      continue;
    }
    if (t.sp == kNfDone) {
      const uint32_t before = lc.node_visits;
      nf_finish<true>(in, t, lc);
      st.loads += 2 * (lc.node_visits - before);  // the reference boxes it tested
      if (!t.done) trav_fetch(in, t);
      continue;
    }
    const bool in_inst = t.ret != kNoRet && (t.ret & kRetInstance);
    if (trav_at_box(t)) {
      st.loads += 2;
      trav_box_index_either<true, true, WILD>(in, stk, t, lc);
    } else {
      const uint32_t kind = t.s1.w;
      if (kind == KIND_TRI || kind == KIND_SPHERE) {
        st.loads += kind == KIND_TRI ? 3 : 2;
        st.prims++;
      } else if (kind == KIND_INST && t.s0.w != 0 && !nf_wild_enter(in, t, t.s0.w)) {
        st.loads += 4, st.wild_skips++;  // the WILD entry, then the leaf's next
      } else if (kind == KIND_INST || kind == KIND_MODEL) {
        st.loads += kind == KIND_INST ? 5 : 2;
        if (kind == KIND_INST) st.entries++;
      } else {
        fprintf(stderr, "nf: unsupported kind %u at %u\n", kind, t.i);
        exit(2);
      }
      trav_prim_index_either<true, ALPHA, false, false, false, true, WILD>(in, stk, t, lc);
    }
    if (in_inst && t.ret == kNoRet) st.loads += 2;  // the step left an instance: the world ray again
    if (!nf_parked<WILD>(t) && t.sp > kNfStack - (WILD ? 0u : 1u)) {  // k_trace's LDS words per lane (launch_trace)
      fprintf(stderr, "nf: stack overflow\n");
      exit(3);
    }
    if (trav_may_fetch<true, WILD>(t)) trav_fetch(in, t);
  }
  st.boxes += lc.node_visits;
  fallbacks += lc.vnf_fallbacks;
  return trav_hit(in, t);
}

template <uint32_t ALPHA>
Hit walk_nf(const Scene& c, V o, V d, Stats& st, uint64_t& fallbacks, uint64_t& starts_ref) {
  return c.S.nf_wild_root != 0 ? walk_nf_w<ALPHA, true>(c, o, d, st, fallbacks, starts_ref)
                               : walk_nf_w<ALPHA, false>(c, o, d, st, fallbacks, starts_ref);
}

bool same_hit(const Hit& r, const Hit& q) {
  return r.prim == q.prim && r.container == q.container && (r.prim == kRefNone || f2u(r.t) == f2u(q.t));
}

// n x 6 float32 rays of a file
bool read_rays(const char* path, std::vector<float>& rays) {
  FILE* f = fopen(path, "rb");
  if (!f) return fprintf(stderr, "cannot read %s\n", path), false;
  float buf[6 * 1024];
  for (size_t k; (k = fread(buf, sizeof(float), 6 * 1024, f)) > 0;) rays.insert(rays.end(), buf, buf + k);
  fclose(f);
  return true;
}

// `hits` / `hits-nf`: k_rays_in -> walk -> k_rays_out on the host
// world: the scene is a world file's — the walk's statistics are printed, and
// starts_path (if any) gets a byte per ray: 1, the ray started near first
template <uint32_t ALPHA>
int trace_file(const Scene& c, bool nf, const char* rays_path, const char* out_path, const char* name, bool world,
               const char* starts_path) {
  std::vector<float> rays;
  if (!read_rays(rays_path, rays)) return 1;
  const size_t n = rays.size() / 6;
  std::vector<uint32_t> out(4 * n);
  std::vector<uint8_t> near_first(n, 0);
  Stats st;
  uint64_t fb = 0, sr = 0;
  for (size_t i = 0; i < n; ++i) {
    const float* r = &rays[6 * i];
    const V o{r[0], r[1], r[2]}, d{r[3], r[4], r[5]};
    const uint64_t sr0 = sr;
    const Hit h = nf ? walk_nf<ALPHA>(c, o, d, st, fb, sr) : walk_ref<ALPHA>(c, o, d);
    near_first[i] = nf && sr == sr0;
    const bool hit = h.prim != kRefNone;
    out[4 * i] = h.prim;
    out[4 * i + 1] = h.container;
    out[4 * i + 2] = hit ? f2u(h.t) : 0u;
    out[4 * i + 3] = hit && resolve_hit(c.S, o, d, h).front_face ? 1u : 0u;
  }
  FILE* f = fopen(out_path, "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return fprintf(stderr, "cannot write %s\n", out_path), 1;
  fclose(f);
  if (world)
    printf("%-14s %s: %zu rays, fallbacks %llu, starts_ref %llu\n", name, nf ? "hits-nf" : "hits", n,
           (unsigned long long)fb, (unsigned long long)(nf ? sr : n));
  if (starts_path) {
    f = fopen(starts_path, "wb");
    if (!f || fwrite(near_first.data(), 1, n, f) != n) return fprintf(stderr, "cannot write %s\n", starts_path), 1;
    fclose(f);
  }
  return 0;
}

template <uint32_t ALPHA>
int run(int argc, char** argv, const mrt_scene_desc& d, const mrt_camera& cam, HostScene& s) {
  int n = argc > 2 ? atoi(argv[2]) : 20000;
  const char* mode = argc > 4 ? argv[4] : "";
  std::string err;
  const bool hits_nf = !strcmp(mode, "hits-nf");
  if (hits_nf || !strcmp(mode, "hits")) {
    if (argc < 7) return fprintf(stderr, "%s <rays.f32> <out.u32>\n", mode), 1;
    if (hits_nf && !s.nf_ok) return fprintf(stderr, "%s: no near-first trees (%s)\n", argv[1], s.nf_note.c_str()), 1;
    const bool world = argv[1][0] == '@';
    return trace_file<ALPHA>(Scene(s), hits_nf, argv[5], argv[6], argv[1], world, world && argc > 7 ? argv[7] : nullptr);
  }
  // `bound` mode: the double-precision bound checks (check_hit, check_hit_wild, the cones) on the rays of a
  // file instead of the camera and bounce rays below
  const bool bound = !strcmp(mode, "bound");
  std::vector<float> file_rays;
  if (bound && (argc < 6 || !read_rays(argv[5], file_rays))) return fprintf(stderr, "bound <rays.f32>\n"), 1;
  if (bound) n = (int)(file_rays.size() / 6);
  // `layout` mode: the same rays through the plain preorder stream (build_host_scene(..., false))
  // and the default layout (BLAS regions with siblings together) must find the
  // same closest hits, t bits included, after the same number of box tests
  HostScene dfs;
  const bool layout = !strcmp(mode, "layout");
  // `nf` mode: the verified near-first walk must find the reference's closest
  // hits (primitive, container, t bits) on every ray
  const bool nf = !strcmp(mode, "nf") || !strcmp(mode, "graze") || !strcmp(mode, "tangent") || bound;
  // `graze` mode: rays nearly parallel to a triangle of the scene (angle
  // 10^U(-8,-1.5) rad to its plane, through a random point of it, from 0.5-60
  // units back; through an instance's transform half the time) — where
  // Moller-Trumbore's t is least accurate, the near-first walk's culling
  // margin is tested hardest
  const bool graze = !strcmp(mode, "graze");
  // `tangent` mode: rays nearly tangent to a sphere (offset 10^U(-7,-1) of its
  // radius from the tangent line) from 1-400 radii away — where the sphere
  // test's disc cancels
  const bool tangent = !strcmp(mode, "tangent");
  if (getenv("SLAB_ZERO_RHO")) {  // experiment: the walk without its rounding margins (not exact)
    const float wr = s.nfb.wr;
    s.nfb = NfBound{};
    s.nfb.sr = -1.0f;
    s.nfb.wr = wr;
  }
  if (getenv("SLAB_GEN_SCALE")) s.nfb.aw1 *= atof(getenv("SLAB_GEN_SCALE"));
  if (nf && s.nf_ok) {
    const NfBound& B = s.nfb;
    printf("%-14s bound: aw0 %.3g aw1 %.3g bw0 %.3g bw1 %.3g kw1 %.3g ko1 %.3g ao0 %.3g ao1 %.3g orad %.3g | world ball r %.3g"
           " generic r %.3g | spheres r %.3g s51 %.3g s11 %.3g | generic triangles %u off every coordinate plane, %u on one\n",
           argv[1], B.aw0, B.aw1, B.bw0, B.bw1, B.kw1, B.ko1, B.ao0, B.ao1, B.orad, B.wr, B.gr, B.sr, B.s51, B.s11, s.nf_generic,
           s.nf_generic_planar);
  }
  if (nf && !s.nf_ok) {
    printf("%-14s nf: no near-first trees (%s)\n", argv[1], s.nf_note.c_str());
    return 0;
  }
  if (nf && s.nf_ok) {  // NF parents for the cone-narrowed bound checks
    g_leaf_parent.assign(s.vnf_leaf.size() / 2, ~0u);
    std::vector<uint8_t> seen(s.slots.size() / 4, 0);
    map_nf_tree(s, s.nf_world, seen);
    if (s.nf_wild_root) map_nf_tree(s, s.nf_wild_root, seen);  // the wild instances' own tree (layout.h)
    printf("%-14s nf cones: %u of %u nodes carry one, kc %.3g\n", argv[1], s.nf_cones, s.nf_boxes, (double)s.nfb.kc);
    for (const auto& [inst, at] : g_wild_entry) {
      const NfWild e = wild_entry(s, at);
      printf("%-14s wild instance %u: box (%.4g %.4g %.4g)-(%.4g %.4g %.4g) a0 %.3g a1 %.3g b0 %.3g b1 %.3g r %.3g\n", argv[1],
             inst, e.mn[0], e.mn[1], e.mn[2], e.mx[0], e.mx[1], e.mx[2], e.a0, e.a1, e.b0, e.b1, e.r);
    }
  }
  const Scene scn(s);  // after the experiments above: it carries s.nfb
  uint64_t nf_bad = 0, nf_fallbacks = 0, nf_starts_ref = 0, nf_even = 0, nf_odd = 0;
  BoundCheck bc;
  if (nf) g_bc = &bc;
  std::vector<uint32_t> nf_per_ray, ref_per_ray;  // box tests per ray: the tail a persistent wave waits on
  Stats nf_st;
  if (layout) {
    if (!build_host_scene(d, dfs, err, false)) return 1;
  }
  const Scene scn_dfs(dfs);
  uint64_t layout_bad = 0;
  std::mt19937 g(7);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  Stats st;
  uint64_t hits = 0, fast = 0;
  const V o{cam.origin[0], cam.origin[1], cam.origin[2]};
  V cam_d{0, 0, -1};
  for (int k = 0; k < n; ++k) {
    V ro, rd;
    if (bound) {
      const float* r = &file_rays[6 * (size_t)k];
      ro = {r[0], r[1], r[2]}, rd = {r[3], r[4], r[5]};
    } else if (tangent) {
      if (!d.n_spheres) break;
      const mrt_sphere& sp = d.spheres[std::min<uint32_t>(d.n_spheres - 1, (uint32_t)(u(g) * d.n_spheres))];
      const float rad = fabsf(sp.radius);
      V w{u(g) * 2 - 1, u(g) * 2 - 1, u(g) * 2 - 1};
      const float wl = sqrtf(dot(w, w));
      if (!(wl > 0.1f)) continue;
      w = {w.x / wl, w.y / wl, w.z / wl};  // from the centre towards the tangent point
      V t1 = cross(w, fabsf(w.x) < 0.9f ? V{1, 0, 0} : V{0, 1, 0});
      const float tl = sqrtf(dot(t1, t1));
      t1 = {t1.x / tl, t1.y / tl, t1.z / tl};
      const float off = rad * (1.0f + (u(g) < 0.5f ? -1.0f : 1.0f) * powf(10.0f, -7.0f + 6.0f * u(g)));
      const V p{sp.center[0] + w.x * off, sp.center[1] + w.y * off, sp.center[2] + w.z * off};
      const float sc = 0.5f + 1.5f * u(g), back = rad * powf(10.0f, 2.6f * u(g));
      rd = {t1.x * sc, t1.y * sc, t1.z * sc};
      ro = {p.x - rd.x * back / sc, p.y - rd.y * back / sc, p.z - rd.z * back / sc};
    } else if (graze) {
      const mrt_triangle& tr = d.triangles[std::min<uint32_t>(d.n_triangles - 1, (uint32_t)(u(g) * d.n_triangles))];
      const float* m = nullptr;
      if (d.n_instances && u(g) < 0.5f)
        m = d.instances[std::min<uint32_t>(d.n_instances - 1, (uint32_t)(u(g) * d.n_instances))].fwd;
      auto xw = [&](const float* v, float w) -> V {
        if (!m) return {v[0] * w + (1 - w) * v[0], v[1], v[2]};
        return {m[0] * v[0] + m[4] * v[1] + m[8] * v[2] + m[12] * w, m[1] * v[0] + m[5] * v[1] + m[9] * v[2] + m[13] * w,
                m[2] * v[0] + m[6] * v[1] + m[10] * v[2] + m[14] * w};
      };
      const V A = xw(tr.a, 1), B = xw(tr.b, 1), C = xw(tr.c, 1);
      float b1 = u(g), b2 = u(g);
      if (b1 + b2 > 1) b1 = 1 - b1, b2 = 1 - b2;
      const V p{A.x + (B.x - A.x) * b1 + (C.x - A.x) * b2, A.y + (B.y - A.y) * b1 + (C.y - A.y) * b2,
                A.z + (B.z - A.z) * b1 + (C.z - A.z) * b2};
      V nn = cross(B - A, C - A);
      const double nl = sqrt((double)dot(nn, nn));
      if (!(nl > 0)) continue;
      nn = {(float)(nn.x / nl), (float)(nn.y / nl), (float)(nn.z / nl)};
      V t1 = cross(nn, fabsf(nn.x) < 0.9f ? V{1, 0, 0} : V{0, 1, 0});
      const float tl = sqrtf(dot(t1, t1));
      t1 = {t1.x / tl, t1.y / tl, t1.z / tl};
      const V t2 = cross(nn, t1);
      const float phi = 6.2831853f * u(g), th = powf(10.0f, -8.0f + 6.5f * u(g)) * (u(g) < 0.5f ? -1.0f : 1.0f);
      const float sc = 0.5f + 1.5f * u(g), back = 0.5f + 59.5f * u(g);
      const float ct = cosf(th), st_ = sinf(th);
      rd = {sc * (ct * (cosf(phi) * t1.x + sinf(phi) * t2.x) + st_ * nn.x),
            sc * (ct * (cosf(phi) * t1.y + sinf(phi) * t2.y) + st_ * nn.y),
            sc * (ct * (cosf(phi) * t1.z + sinf(phi) * t2.z) + st_ * nn.z)};
      ro = {p.x - rd.x * back, p.y - rd.y * back, p.z - rd.z * back};
    } else if (k % 2 == 0) {  // camera ray
      const float s1 = u(g), t1 = u(g);
      rd = {((cam.lower_left_corner[0] + cam.horizontal[0] * s1) + cam.vertical[0] * t1) - o.x,
            ((cam.lower_left_corner[1] + cam.horizontal[1] * s1) + cam.vertical[1] * t1) - o.y,
            ((cam.lower_left_corner[2] + cam.horizontal[2] * s1) + cam.vertical[2] * t1) - o.z};
      ro = o;
      cam_d = rd;
    } else {  // from the first hit of the previous camera ray, random direction (a bounce)
      const Hit h = walk_ref<ALPHA>(scn, o, cam_d);
      if (h.prim == kRefNone) continue;
      ro = {o.x + cam_d.x * h.t, o.y + cam_d.y * h.t, o.z + cam_d.z * h.t};
      rd = {u(g) * 2 - 1, u(g) * 2 - 1, u(g) * 2 - 1};
    }
    fast += tray_fast(make_tray(ro, rd, scn.S.fast_ok));
    const uint64_t boxes0 = st.boxes;
    // a file's ray is checked where the bound is claimed: if it starts near first (nf_bound.h nf_ray_ok)
    bool covered = true;
    if (bound) {
      Stats probe;
      uint64_t fb = 0, sr = 0;
      walk_nf<ALPHA>(scn, ro, rd, probe, fb, sr);
      covered = sr == 0;
    }
    const Hit r = walk_ref<ALPHA>(scn, ro, rd, &st, covered);
    hits += r.prim != kRefNone;
    if (nf) {
      const uint64_t nb0 = nf_st.boxes;
      const Hit q = walk_nf<ALPHA>(scn, ro, rd, nf_st, nf_fallbacks, nf_starts_ref);
      nf_per_ray.push_back(uint32_t(nf_st.boxes - nb0));
      (k % 2 ? nf_odd : nf_even) += nf_st.boxes - nb0;
      ref_per_ray.push_back(uint32_t(st.boxes - boxes0));
      const bool bad = !same_hit(r, q);
      if (bad && nf_bad < 5)
        fprintf(stderr, "nf differs: ref prim %08x cont %08x t %a | nf prim %08x cont %08x t %a\n", r.prim, r.container,
                r.t, q.prim, q.container, q.t);
      nf_bad += bad;
    }
    if (layout) {
      Stats sd;
      const Hit q = walk_ref<ALPHA>(scn_dfs, ro, rd, &sd);
      layout_bad += r.prim != q.prim || r.container != q.container || f2u(r.t) != f2u(q.t) || sd.boxes != st.boxes - boxes0;
    }
  }
  if (nf) {
    printf("%-14s nf: %llu of %d rays differ from the reference walk; box tests %.1f vs %.1f per ray (x%.2f), "
           "record loads %.1f vs %.1f (x%.2f), %llu fallbacks (%.2f%%), stack need %u\n",
           argv[1], (unsigned long long)nf_bad, n, (double)nf_st.boxes / n, (double)st.boxes / n,
           (double)st.boxes / std::max<uint64_t>(nf_st.boxes, 1), (double)nf_st.loads / n, (double)st.loads / n,
           (double)st.loads / std::max<uint64_t>(nf_st.loads, 1), (unsigned long long)nf_fallbacks,
           100.0 * nf_fallbacks / n, s.nf_stack_need);
    auto tail = [](std::vector<uint32_t> v, double q) {
      if (v.empty()) return 0u;
      std::sort(v.begin(), v.end());
      return v[std::min<size_t>(v.size() - 1, size_t(q * v.size()))];
    };
    printf("%-14s nf tail: box tests per ray p99 %u / p99.9 %u / max %u (reference walk %u / %u / %u)\n", argv[1],
           tail(nf_per_ray, 0.99), tail(nf_per_ray, 0.999), tail(nf_per_ray, 1.0), tail(ref_per_ray, 0.99),
           tail(ref_per_ray, 0.999), tail(ref_per_ray, 1.0));
    printf("%-14s nf bound: %llu accepted hits checked, %llu outside their box, worst dist/rho %.3g, %llu over; "
           "%llu rays start on the reference walk (%.2f%%), %u wild instances\n",
           argv[1], (unsigned long long)bc.checks, (unsigned long long)bc.outside, bc.worst,
           (unsigned long long)bc.over, (unsigned long long)nf_starts_ref, 100.0 * nf_starts_ref / n, s.nf_wild);
    printf("%-14s nf box tests per ray: even rays %.1f, odd rays %.1f; instance entries per ray %.3f\n", argv[1],
           2.0 * nf_even / n, 2.0 * nf_odd / n, (double)nf_st.entries / n);
    printf("%-14s nf wild instances passed by per ray %.3f; primitive tests per ray %.2f; cost estimate %.0f VALU/ray "
           "(58 per box test, 45 per primitive test, 500 per instance entry)\n", argv[1], (double)nf_st.wild_skips / n,
           (double)nf_st.prims / n, (58.0 * nf_st.boxes + 45.0 * nf_st.prims + 500.0 * nf_st.entries) / n);
    printf("%-14s reference walk: instance entries per ray %.3f\n", argv[1], (double)st.entries / n);
    printf("%-14s nf wild: %llu hits of wild instances checked, worst dist/rho %.3g\n", argv[1],
           (unsigned long long)bc.wild_checks, bc.worst_wild);
    if (bc.over) return 1;
    if (nf_bad) return 1;
  }
  if (layout) {
    printf("%-14s layout: %llu of %d rays differ between the sibling layout and the preorder stream; stream %zu vs %zu slots\n",
           argv[1], (unsigned long long)layout_bad, n, s.slots.size() / 4, dfs.slots.size() / 4);
    if (layout_bad) return 1;
  }
  printf("%-14s rays %d (early domain %llu) hits %llu  boxes %llu  left to the exact test %.5f  wrong %llu\n", argv[1],
         n, (unsigned long long)fast, (unsigned long long)hits, (unsigned long long)st.boxes,
         (double)st.undecided / std::max<uint64_t>(st.boxes, 1), (unsigned long long)st.wrong);
  return st.wrong ? 1 : 0;
}

// `stream` mode: what the host builds for the device, as element counts and
// 64-bit FNV-1a hashes — the record stream and its tables under both layouts,
// and the treelet at several budgets (slots). A change of the host code that
// must leave the stream alone is checked by comparing these lines before and
// after; the function reads HostScene's public fields only, so the same text
// compiles against either side of such a change.
int stream_mode(const char* scene, mrt_builder* b, const mrt_scene_desc& d) {
  mrt_scene_ext ext{};
  const mrt_volume_target* targets = nullptr;
  uint32_t n_targets = 0;
  mrt_builder_desc_ext(b, &ext);
  mrt_builder_volume_targets(b, &targets, &n_targets);
  // columns: scene, layout, item, treelet budget (-: none), elements, hash, the value of a scalar (-: an array)
  auto line = [&](const char* layout, const char* item, long budget, const void* p, size_t n, size_t elem, bool scalar) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t k = 0; k < n * elem; ++k) h = (h ^ static_cast<const uint8_t*>(p)[k]) * 0x100000001b3ull;
    char bud[24] = "-", val[24] = "-";
    if (budget >= 0) snprintf(bud, sizeof bud, "%ld", budget);
    if (scalar) snprintf(val, sizeof val, "%u", *static_cast<const uint32_t*>(p));
    printf("%-18s %-8s %-14s %8s %10zu %016llx %s\n", scene, layout, item, bud, n, (unsigned long long)h, val);
  };
  for (const bool sibling : {true, false}) {
    const char* L = sibling ? "sibling" : "preorder";
    HostScene s;
    s.nf_build = kNfBuildAlways;
    std::string err;
    if (!build_host_scene(d, s, err, sibling, &ext, targets, n_targets)) return printf("%s: %s\n", scene, err.c_str()), 1;
    auto vec = [&](const char* item, const std::vector<uint32_t>& v, long budget = -1) {
      line(L, item, budget, v.data(), v.size(), 4, false);
    };
    auto one = [&](const char* item, uint32_t v, long budget = -1) { line(L, item, budget, &v, 1, 4, true); };
    vec("slots", s.slots);
    vec("rec_starts", s.rec_starts);
    vec("vnf_leaf", s.vnf_leaf);
    std::vector<uint32_t> regions;
    for (const BlasRegion& r : s.blas_regions) regions.insert(regions.end(), {r.begin, r.end, r.refs, r.model ? 1u : 0u});
    line(L, "blas_regions", -1, regions.data(), s.blas_regions.size(), 16, false);
    one("world_begin", s.world_begin);
    one("world_end", s.world_end);
    one("nf_ok", s.nf_ok ? 1u : 0u);
    one("nf_world", s.nf_world);
    one("nf_wild_root", s.nf_wild_root);
    one("nf_first_slot", s.nf_first_slot);
    line(L, "vnf_base", -1, s.vnf_base, 4, 4, false);
    const long whole = (long)(s.slots.size() / 4);  // a budget the whole stream fits
    for (const long budget : {0l, 64l, 1536l, 4992l, whole}) {
      build_treelet(s, (uint32_t)budget);
      vec("tlet", s.tlet, budget);
      vec("slots_tl", s.slots_tl, budget);
      one("tl_world_begin", s.tl_world_begin, budget);
      one("tl_boxes", s.tl_boxes, budget);
    }
  }
  return 0;
}

// A world file (tests/adversarial_worlds.py write()): whitespace-separated words, every float a C hex float.
//   seed <n>                          first: the builder's seed (the reference's tree, and with it its closest
//                                     hit on a 0/0 slab, depends on the builder's draws)
//   sphere <c: 3> <r>
//   tri <abc: 9>
//   model <add_to_world: 0|1> <n> <n x 9>
//   instance <model: its number among the file's models> <translation: 3> <rotation: 3> <scale: 3>
//   camera <vfov> <look_from: 3> <look_at: 3>      (aspect 16:9)
// One grey Lambertian material for everything, as the Python builders of the same ops use. The tree is built
// after the last word.
mrt_builder* load_world(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return fprintf(stderr, "cannot read %s\n", path), nullptr;
  char word[32];
  auto floats = [&](float* v, size_t n) {
    for (size_t k = 0; k < n; ++k)
      if (fscanf(f, "%a", &v[k]) != 1) return false;
    return true;
  };
  unsigned long long seed = 0;
  if (fscanf(f, "%31s %llu", word, &seed) != 2 || strcmp(word, "seed")) return fprintf(stderr, "%s: no seed\n", path), nullptr;
  mrt_builder* b = nullptr;
  mrt_builder_new(seed, &b);
  const uint32_t mat = (uint32_t)mrt_builder_material(b, MRT_MAT_LAMBERTIAN, (uint32_t)mrt_builder_solid(b, 0.5f, 0.5f, 0.5f, 1.0f),
                                                      0.0f, 0.0f, 0.0f, 0.0f);
  std::vector<int> models;
  bool ok = true;
  while (ok && fscanf(f, "%31s", word) == 1) {
    float v[10];
    if (!strcmp(word, "sphere")) {
      ok = floats(v, 4) && mrt_builder_add_sphere(b, mat, v[0], v[1], v[2], v[3]) == 0;
    } else if (!strcmp(word, "tri")) {
      ok = floats(v, 9) && mrt_builder_add_triangle(b, mat, v) == 0;
    } else if (!strcmp(word, "model")) {
      unsigned add = 0, n = 0;
      ok = fscanf(f, "%u %u", &add, &n) == 2 && n > 0 && n < (1u << 20);
      std::vector<float> tris(ok ? 9 * (size_t)n : 0);
      ok = ok && floats(tris.data(), tris.size());
      if (ok) models.push_back(mrt_builder_model(b, mat, 0xFFFFFFFFu, tris.data(), n, 0, (int)add));
      ok = ok && models.back() >= 0;
    } else if (!strcmp(word, "instance")) {
      unsigned m = 0;
      ok = fscanf(f, "%u", &m) == 1 && m < models.size() && floats(v, 9) &&
           mrt_builder_add_instance(b, models[m], v, v + 3, v + 6, 0xFFFFFFFFu) == 0;
    } else if (!strcmp(word, "camera")) {
      const float up[3] = {0, 1, 0};
      ok = floats(v, 7);
      const float e[3] = {v[1] - v[4], v[2] - v[5], v[3] - v[6]};
      ok = ok && mrt_builder_camera(b, v[0], v + 1, v + 4, up, 16.0f / 9.0f, 0.0f, sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])) == 0;
    } else {
      ok = false;
    }
  }
  fclose(f);
  if (!ok) {
    fprintf(stderr, "%s: cannot use `%s` (%s)\n", path, word, mrt_builder_last_error());
    mrt_builder_free(b);
    return nullptr;
  }
  return b;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  mrt_builder* b = nullptr;
  if (argv[1][0] == '@') {  // a world file
    if (!(b = load_world(argv[1] + 1))) return 1;
  } else {
    mrt_builder_new(1, &b);
    if (mrt_builder_builtin(b, argv[1], 16.0f / 9.0f, argc > 3 ? argv[3] : "tests/golden") != 0) {
      printf("%s: %s\n", argv[1], mrt_global_last_error());
      return 1;
    }
  }
  mrt_builder_build_bvh(b);
  mrt_scene_desc d;
  mrt_camera cam;
  mrt_builder_desc(b, &d, &cam);
  if (argc > 4 && !strcmp(argv[4], "stream")) {  // every scene, those whose traversal draws random numbers too
    const int rc = stream_mode(argv[1], b, d);
    mrt_builder_free(b);
    return rc;
  }
  HostScene s;
  s.keep_nf_boxes = true;  // the bound checks' leaf boxes
  s.nf_build = kNfBuildAlways;  // the trees even where the per-scene rule would walk the reference's way
  std::string err;
  if (!build_host_scene(d, s, err)) {
    printf("%s\n", err.c_str());
    return 1;
  }
  if (s.trav_rng) {  // Volume, Mix alpha tests: the walks here carry no random stream
    printf("%s: the scene's traversal draws random numbers; not supported\n", argv[1]);
    return 2;
  }
  // alpha tests the way the library chooses its k_trace variant (trace.hip launch_trace)
  const bool ext = !s.surf_ops.empty() || s.bg_kind == MRT_BG_CUBEMAP;
  const int rc = !s.has_alpha ? run<0>(argc, argv, d, cam, s) : ext ? run<2>(argc, argv, d, cam, s) : run<1>(argc, argv, d, cam, s);
  mrt_builder_free(b);
  return rc;
}
