// walk.h — the reference's walk, one record per step: the per-lane state, the
// record loads, the box and primitive steps over the preorder stream
// (layout.h), the whole traversal of one ray.
//   World::intersect      world.rs:131-144
//   BvhNode::intersect    geom.rs:185-205 (via the preorder stream, layout.h)
//   Instance::intersect   geom.rs:403-420
//   Volume::intersect     geom.rs:609-653
#pragma once
#include "isect.h"

namespace mrt {

struct Hit {
  float t;
  uint32_t prim;       // make_ref(kind, id) or kRefNone
  uint32_t container;  // make_ref(INSTANCE|MODEL, id) or kRefNone
};

// World::intersect over the preorder stream, one record per step so that a
// persistent kernel can interleave many rays per lane (trace.hip k_trace).
// Each lane's sequence of box/primitive tests is exactly the reference's
// (left-first recursion with shrinking t_max, geom.rs:185-205); only which
// lanes of a wave are busy at a time differs.
//
// Register budget: the per-lane state is kept small (occupancy is the lever
// for this latency-bound loop). The world ray is not kept: the rays live in
// the pool buffers (ro/rd), and leaving an instance's BLAS reloads it. The
// closest t so far is `best` (Hit.t is filled in by trav_hit()).
struct TravIn {
  const DevScene& S;
  const uint4* slots;      // record stream in global memory (S.slots, or S.slots_tl beside an LDS treelet)
  uint32_t world_begin;    // first record of the world region (an LDS-tagged index beside a treelet)
  const float4* ro;        // ray origins  (xyz) of the pool
  const float4* rd;        // ray directions (xyz)
  float tmin;
  uint4* rng = nullptr;    // the rays' RNG states (traversal draws: Volume, Mix alpha tests)
  float tmax0 = INFINITY;  // the walk's initial t_max (a near-first lane that falls back restarts with it)
  // k_trace (reference walk, no treelet): this lane's 4 x 16 B of LDS, stride
  // `stash_stride` float4s, holding the world ray while the lane is inside an
  // instance's BLAS — leaving it then costs 4 LDS reads instead of 2 pool
  // loads and make_tray's four correctly rounded divisions (nullptr: recompute)
  float4* stash = nullptr;
  uint32_t stash_stride = 0;
};
MRT_HD void tray_stash(const TravIn& in, const TRay& r) {
  float4* p = in.stash;
  const uint32_t k = in.stash_stride;
  p[0] = make_float4(r.o.x, r.o.y, r.o.z, r.d.x);
  p[k] = make_float4(r.d.y, r.d.z, r.yx, r.yy);
  p[2 * k] = make_float4(r.yz, r.oyx, r.oyy, r.oyz);
  p[3 * k] = make_float4(r.om, r.a.b, r.a.y, 0.0f);
}
MRT_HD TRay tray_unstash(const TravIn& in) {
  const float4* p = in.stash;
  const uint32_t k = in.stash_stride;
  const float4 a = p[0], b = p[k], c = p[2 * k], e = p[3 * k];
  TRay r;
  r.o = V3{a.x, a.y, a.z};
  r.d = V3{a.w, b.x, b.y};
  r.yx = b.z, r.yy = b.w, r.yz = c.x;
  r.oyx = c.y, r.oyy = c.z, r.oyz = c.w;
  r.om = e.x;
  r.a.b = e.y, r.a.y = e.z;
  return r;
}
// A path's stream (mrt_rng.h PathRng) as the pool keeps it: s0 and s1, low word first.
MRT_HD PathRng rng_unpack(uint4 q) {
  return PathRng{(unsigned long long)q.x | ((unsigned long long)q.y << 32),
                 (unsigned long long)q.z | ((unsigned long long)q.w << 32)};
}
MRT_HD uint4 rng_pack(PathRng g) {
  return make_uint4((uint32_t)g.s0, (uint32_t)(g.s0 >> 32), (uint32_t)g.s1, (uint32_t)(g.s1 >> 32));
}

// Inside a BLAS, `ret` is the world record after the instance/model record
// that entered it, with kRetInstance set for an instance; the container of a
// hit is recovered from that record when the ray finishes (trav_hit).
constexpr uint32_t kNoRet = 0xFFFFFFFFu;
constexpr uint32_t kRetInstance = 0x80000000u;
constexpr uint32_t kExactMode = 0xFFFDu;  // Trav::sp of the reference's walk (below walk_nf.h's kNfWait, kNfDone)

struct Trav {
  TRay r;  // ray of the space being traversed (world, or instance object space)
  uint32_t ray;  // pool index of the ray
  uint32_t i, ret;
  float best;
  uint32_t prim, hit_ret;  // closest hit so far: primitive (kRefNone: none) and `ret` when found
  uint4 s0, s1;  // current record (prefetched when i moves)
  PathRng rng;   // the ray's stream, for scenes whose traversal draws (RNG variants only)
  uint32_t sp;   // near-first walk: stack entries in use (kExactMode: the reference's walk)
  float t2;      // near-first walk: the smallest t of the other hits it met (nf_finish)
  NfLine nfl;    // near-first walk: the current space's rounding margin, for t <= cull(best) (nf_bound.h nf_line)
  float nl;      // near-first walk: the current node's hits have t <= nl (its box's exit; +inf: unknown)
  bool done;
#ifdef MRT_DEBUG_BOUNDS
  uint32_t steps;
#endif
};

// LDS treelet (layout.h): records with kLdsTag in their index live in the
// workgroup's LDS copy (mrt_lds), the rest in the global stream. Kernels
// built with LDS=false never see a tagged index, nor does the host (which
// has no LDS: the tagged branch exists on the device only).
extern __shared__ uint4 mrt_lds[];
template <bool LDS>
MRT_HD void rec_load2(const TravIn& in, uint32_t i, uint4& a, uint4& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (LDS && (i & kLdsTag)) {
    const uint32_t j = i & kIdxMask;
    a = mrt_lds[MRT_IDX(in.S, j, in.S.n_tlet, 22)];
    b = mrt_lds[MRT_IDX(in.S, j + 1, in.S.n_tlet, 22)];
  } else
#endif
  {
    (void)MRT_IDX(in.S, i + 1, in.S.n_slots, 6);
    const uint4* p = in.slots + MRT_IDX(in.S, i, in.S.n_slots, 5);  // one address, offset:16 for slot 2
    a = p[0];
    b = p[1];
  }
}
template <bool LDS>
MRT_HD uint4 rec_load1(const TravIn& in, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (LDS && (i & kLdsTag)) return mrt_lds[MRT_IDX(in.S, i & kIdxMask, in.S.n_tlet, 22)];
#endif
  return in.slots[MRT_IDX(in.S, i, in.S.n_slots, 7)];
}

template <bool LDS = false>
MRT_HD Hit trav_hit(const TravIn& in, const Trav& t) {
  uint32_t container = kRefNone;
  if (t.hit_ret != kNoRet) {
    const uint32_t rec = (t.hit_ret & ~kRetInstance) - 2;  // the instance/model record
    container = make_ref((t.hit_ret & kRetInstance) ? MRT_REF_INSTANCE : MRT_REF_MODEL, rec_load1<LDS>(in, rec).x);
  }
  return Hit{t.best, t.prim, container};
}

MRT_HD TRay world_ray(const TravIn& in, uint32_t ray) {
  const float4 o4 = in.ro[ray], d4 = in.rd[ray];
  return make_tray(V3{o4.x, o4.y, o4.z}, V3{d4.x, d4.y, d4.z}, in.S.fast_ok);
}
// Entering instance `id` (geom.rs:403-420): ray r through its inverse transform.
MRT_HD TRay instance_ray(const DevScene& S, uint32_t id, const TRay& r) {
  V3 c0, c1, c2, c3;
  load_m12(S.inst_inv + (size_t)MRT_IDX(S, id, S.n_inst, 8) * 12, c0, c1, c2, c3);
  return make_tray(xform(c0, c1, c2, c3, r.o, 1.0f), xform(c0, c1, c2, c3, r.d, 0.0f), S.fast_ok);
}
// Leaving one: the world ray again, from the lane's stash where it has one.
MRT_HD TRay leave_instance(const TravIn& in, uint32_t ray) { return in.stash ? tray_unstash(in) : world_ray(in, ray); }
// A box record's corners, a triangle record's vertex and edges (layout.h).
struct RecBox {
  V3 mn, mx;
};
MRT_HD RecBox rec_box(const uint4& s0, const uint4& s1) {
  return {{u2f(s0.x), u2f(s0.y), u2f(s0.z)}, {u2f(s0.w), u2f(s1.x), u2f(s1.y)}};
}
struct RecTri {
  V3 a, ab, ac;
};
MRT_HD RecTri rec_tri(const uint4& s0, const uint4& s1, const uint4& s2) {
  return {{u2f(s0.x), u2f(s0.y), u2f(s0.z)}, {u2f(s0.w), u2f(s1.x), u2f(s1.y)}, {u2f(s2.x), u2f(s2.y), u2f(s2.z)}};
}

// Load record t.i. Every region ends in an END record (handled by
// trav_prim: leave the BLAS, or finish), so there is no bounds compare here.
template <bool LDS = false>
MRT_HD void trav_fetch(const TravIn& in, Trav& t) {
#ifdef MRT_DEBUG_BOUNDS
  if (++t.steps > (1u << 24)) {  // record and stop instead of looping
    MRT_IDX(in.S, 0xFFFFFFF0u, 0u, 5);
    t.done = true;
    t.s1.w = KIND_END;  // a done lane never holds a box record (k_trace's box run)
    return;
  }
#endif
  rec_load2<LDS>(in, t.i, t.s0, t.s1);
}

// The region ended: leave the BLAS back to the world ray (geom.rs:405-409;
// a model shares the world ray, an instance's object-space ray is replaced),
// or finish the ray.
MRT_HD void trav_end_index(const TravIn& in, Trav& t) {
  if (t.ret == kNoRet) {
    t.done = true;
    return;
  }
  if (t.ret & kRetInstance) t.r = leave_instance(in, t.ray);
  t.i = t.ret & ~kRetInstance;
  t.ret = kNoRet;
}

// ---- the near-first walk's start (walk_nf.h has the walk) -------------------
// its culling bound: best * (1 + 2^-10)
MRT_HD float nf_cull(float best) { return fmaf(fabsf(best), 0x1p-10f, best); }
// t.nfc: the rounding margin's coefficients (nf_bound.h) of the space being
// walked — set when the walk enters a space; nf_rho_at turns them into how
// far a node's boxes are thickened (trav_box_index_nf)
MRT_HD void nf_margin(const TravIn& in, Trav& t) {
  const bool obj = t.ret != kNoRet && (t.ret & kRetInstance);
  const NfBound& B = in.S.nfb;
  const NfCoef c = obj ? nf_coef_object(B, t.r.o, t.r.a.b) : nf_coef_world(B, t.r.o, t.r.a.b);
  t.nfl = nf_line(B, c, nf_cull(t.best), obj ? B.ao0 : B.aw0, obj ? B.ao1 : B.aw1, t.r.a.b, t.r.d);
}
// stack marker: the bottom entry of a near-first ray's stack in a scene with a
// wild tree (layout.h nf_wild_root). Popped, it says that everything else is
// walked and the wild tree waits (walk_nf.h nf_pop, kNfWait).
constexpr uint32_t kNfWildMark = 0x80000001u;
// the lane's stack of record indices (LDS; kNfStack entries, layout.h)
struct NfStack {
  uint32_t* p;  // this lane's entry 0
  uint32_t stride;
};
MRT_HD void nf_push(const NfStack& k, Trav& t, uint32_t v) {
  k.p[t.sp * k.stride] = v;
  t.sp += 1;  // the builder bounds the depth (nf_stack_need <= kNfStack)
}
// A wave-uniform value moved to its vector register here, not before the
// kernel's loop: hoisted, that register is live across the whole of k_trace,
// which sits at its 96-VGPR cap, and a copy went to scratch memory (8 B per
// lane; tools/kernel_resources.sh). Generates no instruction.
#if defined(__HIP_DEVICE_COMPILE__)
#define MRT_PIN_VGPR(x) asm volatile("" : "+v"(x))
#else
#define MRT_PIN_VGPR(x) (void)0
#endif
// the walk starts at the NF world tree (trav_init_nf): rays its bound does not
// cover (nf_bound.h nf_ray_ok: the generic kappa, and the domain the bound is
// proven on — a finite origin within 2^28, |d| in [2^-50, 2^28]) take the
// reference's walk instead, and push nothing. WILD (the scene
// has a wild tree, layout.h nf_wild_root; k_trace's variant for such scenes):
// the ray first pushes kNfWildMark. LIFO order pops it when everything else
// is done, so a wild leaf, which nothing above it culls, has its own box test
// (walk_nf.h nf_wild_enter) run against the `best` of all the rest. Any
// visiting order is exact: culling uses the current `best`, never below the
// final one, so every primitive whose computed t is <= cull(final best) is
// tested. Scenes without a wild tree compile none of this.
template <bool WILD>
MRT_HD void nf_start(const TravIn& in, const NfStack& k, Trav& t) {
  if (nf_ray_ok(in.S.nfb, t.r.o, t.r.a.b)) {
    if (WILD) {
      uint32_t mark = kNfWildMark;
      MRT_PIN_VGPR(mark);
      nf_push(k, t, mark);
      MRT_PIN_VGPR(t.best);  // the margin's cull(t_max) is computed here, per ray, not kept from before the loop
    }
    nf_margin(in, t);
    t.nl = INFINITY;
  } else {
    t.i = in.world_begin;
    t.sp = kExactMode;
  }
}

// Start ray `ray` of the pool (World::intersect(ray, in.tmin, tmax)): on the
// reference's walk (trav_init), or on the near-first walk at record `start`
// with the lane's stack (trav_init_nf).
template <bool RNG, bool LDS, bool NF, bool WILD>
MRT_HD void trav_begin(const TravIn& in, const NfStack& stk, Trav& t, uint32_t ray, float tmax, uint32_t start) {
  if (RNG) t.rng = rng_unpack(in.rng[ray]);
  t.r = world_ray(in, ray);
  t.ray = ray;
  t.i = NF ? start : in.world_begin;  // the near-first walk starts at its own world tree
  t.sp = NF ? 0u : kExactMode;
  t.t2 = INFINITY;
  t.ret = kNoRet;
  t.best = tmax;
  t.prim = kRefNone;
  t.hit_ret = kNoRet;
  t.done = false;
#ifdef MRT_DEBUG_BOUNDS
  t.steps = 0;
#endif
  if (NF) nf_start<WILD>(in, stk, t);
  trav_fetch<LDS>(in, t);
}
template <bool RNG = false, bool LDS = false>
MRT_HD void trav_init(const TravIn& in, Trav& t, uint32_t ray, float tmax) {
  trav_begin<RNG, LDS, false, false>(in, NfStack{nullptr, 0}, t, ray, tmax, 0u);  // no stack: NF = false never touches it
}
template <bool WILD>
MRT_HD void trav_init_nf(const TravIn& in, const NfStack& stk, Trav& t, uint32_t ray, float tmax, uint32_t start) {
  trav_begin<false, false, true, WILD>(in, stk, t, ray, tmax, start);
}

MRT_HD bool trav_at_box(const Trav& t) { return (int32_t)t.s1.w < 0; }  // kBoxFlag (layout.h)

// The current record is a box: test it and move to the next record's index
// (k_trace's box run loads at the top of each step); trav_box also loads it.
template <bool COUNT>
MRT_HD void trav_box_index(const TravIn& in, Trav& t, LocalCounters& lc) {
  if (COUNT) lc.node_visits++;
  const RecBox b = rec_box(t.s0, t.s1);
  t.i = box_hit_any<COUNT>(b.mn, b.mx, t.r, in.tmin, t.best, &lc) ? (t.s1.w & ~kBoxFlag) : t.s1.z;
}
template <bool COUNT, bool LDS = false>
MRT_HD void trav_box(const TravIn& in, Trav& t, LocalCounters& lc) {
  trav_box_index<COUNT>(in, t, lc);
  trav_fetch<LDS>(in, t);
}

// The ray's RNG state back to the pool (RNG variants, when the ray is done).
MRT_HD void trav_store_rng(const TravIn& in, const Trav& t) { in.rng[t.ray] = rng_pack(t.rng); }

// Volume::intersect once entry and exit of the target over the whole line are
// known (geom.rs:623-653): both clipped to [tmin, best], then a distance
// f.ln() * -1/density drawn from the ray's stream — after every early return,
// as there; the ln is looked up (S.ln_table, upload.h) for the exact value of
// the host libm. t.r is the world ray: its length scales the distance, also
// for an instance target (t is shared between the two spaces).
MRT_HD bool volume_scatter(const DevScene& S, const TravIn& in, Trav& t, uint32_t vid, float te, float tx, float& th) {
  if (te < in.tmin) te = in.tmin;
  if (tx > t.best) tx = t.best;
  if (te >= tx) return false;
  if (te < 0.0f) te = 0.0f;
  const float len = sqrtf(length_squared(t.r.d));
  const float inside = (tx - te) * len;
  const uint32_t m = (uint32_t)(t.rng.next() >> 32) >> 9;  // the draw of f32() (mrt_rng.h)
  const float dist = S.ln_table[MRT_IDX(S, m, 1u << 23, 14)] * S.vol_nid[MRT_IDX(S, vid, S.n_vol, 15)];
  if (dist > inside) return false;
  th = te + dist / len;
  return true;
}

// Volume::intersect with a sphere target (geom.rs:609-622): entry and exit of
// the target over the whole line.
MRT_HD bool volume_hit(const DevScene& S, const TravIn& in, Trav& t, uint4 s0, uint32_t vid, float& th) {
  const V3 c{u2f(s0.x), u2f(s0.y), u2f(s0.z)};
  const float rad = u2f(s0.w);
  float te, tx;
  if (!sphere_hit(c, rad, t.r.o, t.r.d, t.r.a, -INFINITY, INFINITY, te)) return false;
  if (!sphere_hit(c, rad, t.r.o, t.r.d, t.r.a, te + 0.0001f, INFINITY, tx)) return false;
  return volume_scatter(S, in, t, vid, te, tx, th);
}

// The current record is a triangle: Triangle::intersect against [in.tmin,
// t.best], then on to the record after it.
// ALPHA: 0 no alpha tests (the specialisation for scenes without alpha-tested
// triangles: the alpha test's registers would otherwise cost occupancy
// everywhere), 1 alpha tests, 2 alpha tests over EXT surfaces.
template <bool COUNT, uint32_t ALPHA, bool RNG, bool LDS>
MRT_HD void trav_tri_index(const TravIn& in, Trav& t, LocalCounters& lc, uint4 s0, uint4 s1) {
  if (COUNT) lc.triangle_tests++;
  const uint4 s2 = rec_load1<LDS>(in, t.i + 2);
  const RecTri v = rec_tri(s0, s1, s2);
  float th;
  if (tri_hit(v.a, v.ab, v.ac, t.r.o, t.r.d, in.tmin, t.best, th)) {
    const uint32_t id = s1.z & kTriIdMask;
    if (!ALPHA || !(s1.z & kTriAlpha) || tri_alpha_pass<RNG, ALPHA == 2>(in.S, id, t.r.o, t.r.d, th, t.rng, lc)) {
      t.best = th;
      t.prim = make_ref(MRT_REF_TRIANGLE, id);
      t.hit_ret = t.ret;
    }
  }
  t.i = s2.w;
}

// Volume::intersect with an instance or a model as the target (geom.rs:609-
// 622 over Instance::intersect / Model::intersect, 317-328 and 403-420): two
// closest-hit searches of the target's BLAS region, BvhNode::intersect(ray,
// -inf, +inf) and then (ray, enter + 0.0001, +inf); alpha tests of its
// triangles draw from the ray's stream in traversal order, before the
// volume's own draw. The lane that met the record runs both with its own
// Trav, in ONE loop (the second search restarts it: the box and triangle
// steps are inlined once), so nothing but the few words saved here is live
// across them: an instance target's object-space ray replaces t.r (the world
// ray comes back the way leaving an instance brings it back,
// trav_end_index), and best, prim and hit_ret are put back; t.ret stays
// kNoRet throughout (volumes are world objects), t.rng advances by the draws
// made, and t.i / t.s0 / t.s1 are the caller's to set (it holds the record's
// copy). The region holds boxes and triangles and ends in its END record
// (upload.cpp checks that): any other record ends a search, so no stream can
// spin the loop. Counters: what the reference executes — every box and
// triangle test of both searches, one instance / model entry per search.
template <bool COUNT, uint32_t ALPHA, bool LDS>
MRT_HD bool volume_hit_blas(const DevScene& S, const TravIn& in, Trav& t, LocalCounters& lc, uint4 s0, uint4 s1,
                            float& th) {
  const bool inst = s1.z == kVolInstance;
  const float best = t.best;
  const uint32_t prim = t.prim, hit_ret = t.hit_ret;
  if (inst) {
    if (in.stash) tray_stash(in, t.r);
    t.r = instance_ray(S, s0.y, t.r);
  }
  TravIn vin = in;
  vin.tmin = -INFINITY;
  float te = 0.0f;
  bool second = false, hit = false;
  auto start_search = [&]() {
    if (COUNT) (inst ? lc.instance_entries : lc.model_entries)++;
    t.i = s0.x;
    t.best = INFINITY;
    t.prim = kRefNone;
  };
  start_search();
  for (;;) {
    trav_fetch<LDS>(vin, t);
    if (t.done) break;  // MRT_DEBUG_BOUNDS builds: the step cap
    if (trav_at_box(t)) {
      trav_box_index<COUNT>(vin, t, lc);
    } else if (t.s1.w == KIND_TRI) {
      trav_tri_index<COUNT, ALPHA, true, LDS>(vin, t, lc, t.s0, t.s1);
    } else {  // the search is over
      if (t.prim == kRefNone) break;  // enter or exit is None
      hit = second;
      if (second) break;
      second = true;
      te = t.best;
      vin.tmin = te + 0.0001f;
      start_search();
    }
  }
  const float tx = t.best;
  if (inst) t.r = leave_instance(in, t.ray);
  t.best = best;
  t.prim = prim;
  t.hit_ret = hit_ret;
  t.done = false;
  return hit && volume_scatter(S, in, t, s1.x, te, tx, th);
}

// The current record is a primitive, an instance or a model (ALPHA: as for
// trav_tri_index).
// trav_prim_index moves to the next record (or finishes the ray) without
// loading it; trav_prim also loads it.
// VBLAS: the scene may hold volumes whose target is a BLAS (only k_trace tells
// the two apart: the nested searches cost it registers, trace.hip).
template <bool COUNT, uint32_t ALPHA, bool RNG = false, bool LDS = false, bool VBLAS = RNG>
MRT_HD void trav_prim_index(const TravIn& in, Trav& t, LocalCounters& lc) {
  const DevScene& S = in.S;
  const uint4 s0 = t.s0, s1 = t.s1;
  const uint32_t kind = s1.w;
  if (kind == KIND_END) {
    trav_end_index(in, t);
    return;
  }
  if (kind == KIND_TRI) {
    trav_tri_index<COUNT, ALPHA, RNG, LDS>(in, t, lc, s0, s1);
  } else if (kind == KIND_SPHERE) {
    if (COUNT) lc.sphere_tests++;
    float th;
    if (sphere_hit(V3{u2f(s0.x), u2f(s0.y), u2f(s0.z)}, u2f(s0.w), t.r.o, t.r.d, t.r.a, in.tmin, t.best, th)) {
      t.best = th;
      t.prim = make_ref(MRT_REF_SPHERE, s1.x);
      t.hit_ret = t.ret;
    }
    t.i = s1.y;
  } else if (RNG && kind == KIND_VOLUME) {
    float th;
    if (VBLAS && s1.z ? volume_hit_blas<COUNT, ALPHA, LDS>(S, in, t, lc, s0, s1, th) : volume_hit(S, in, t, s0, s1.x, th)) {
      t.best = th;
      t.prim = make_ref(MRT_REF_VOLUME, s1.x);
      t.hit_ret = t.ret;
    }
    t.i = s1.y;
  } else if (kind == KIND_INST) {
    if (COUNT) lc.instance_entries++;
    // entered from the world region: t.r is the world ray here
    if (in.stash) tray_stash(in, t.r);
    t.r = instance_ray(S, s0.x, t.r);
    t.ret = (t.i + 2) | kRetInstance;
    t.i = s0.y;
  } else {  // KIND_MODEL
    if (COUNT) lc.model_entries++;
    t.ret = t.i + 2;
    t.i = s0.y;
  }
}
template <bool COUNT, uint32_t ALPHA, bool RNG = false, bool LDS = false>
MRT_HD void trav_prim(const TravIn& in, Trav& t, LocalCounters& lc) {
  trav_prim_index<COUNT, ALPHA, RNG, LDS>(in, t, lc);
  if (!t.done) trav_fetch<LDS>(in, t);
}

// Whole traversal of pool ray `ray` (one ray per thread); RNG: the
// traversal's draws come from (and advance) `rng`.
template <bool COUNT, bool RNG = false, bool EXT = false>
MRT_HD Hit closest_hit(const TravIn& in, uint32_t ray, float tmax, LocalCounters& lc, PathRng& rng) {
  Trav t;
  trav_init(in, t, ray, tmax);
  if (RNG) t.rng = rng;
  while (!t.done) {
    if (trav_at_box(t))
      trav_box<COUNT>(in, t, lc);
    else
      trav_prim<COUNT, EXT ? 2u : 1u, RNG>(in, t, lc);
  }
  if (RNG) rng = t.rng;
  return trav_hit(in, t);
}

}  // namespace mrt
