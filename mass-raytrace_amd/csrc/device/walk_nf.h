// walk_nf.h — the verified near-first walk (layout.h, nf_tree.cpp;
// k_trace<..., NF>; its start is beside trav_init in walk.h).
// The lane walks the SAH trees near child first with a stack of record
// indices in LDS (kNfStack entries per lane, stride BLK), finds the closest
// hit with the reference's tie rule, then checks that the reference's
// left-first walk reaches that hit; if not it walks again the reference's
// way (sp = kExactMode: trav_box_index / trav_prim_index on the reference
// stream, the exact kernel's steps). Boxes are culled at cull(best) = best *
// (1 + 2^-10), each thickened by rho (nf_bound.h): a bound, proven for the
// reference's own f32 arithmetic, on how far a primitive's computed hit can
// lie outside its box — so the walk meets every primitive whose computed t is
// at most cull(best). Rays the bound does not cover (a
// generic triangle's kappa above kNfKappaMax; an origin that is not finite
// or lies beyond 2^28, |d| outside [2^-50, 2^28]: nf_bound.h nf_ray_ok) take
// the reference's walk.
#pragma once
#include "walk.h"

namespace mrt {

constexpr uint32_t kNfDone = 0xFFFFu;     // Trav::sp: the near-first walk is over, its hit not yet checked
constexpr uint32_t kNfRet = 0x80000000u;  // stack marker: leave the BLAS (back to the world ray)
// Trav::sp: everything but the wild instances' tree is walked; the lane waits
// (holding an END record, as a lane whose walk is over) until k_trace sends a
// batch of such lanes into that tree together (nf_resume_wild)
constexpr uint32_t kNfWait = 0xFFFEu;
// the lane is not stepping: it waits for the wild tree's batch or for its hit's
// check (the two largest values of sp: one compare beside every fetch)
// (WILD false: no lane ever waits, and this is `sp == kNfDone`)
template <bool WILD>
MRT_HD bool nf_parked(const Trav& t) { return WILD ? t.sp >= kNfWait : t.sp == kNfDone; }

// (NfStack and nf_push are beside the walk's start in walk.h, which pushes
// the wild instances' tree before anything else)
// next record from the stack; false: the walk is over. A return marker
// (leaving a BLAS) sits above world entries only — instances are world
// objects, never nested — so one pop meets at most one: straight-line code,
// the marker's branch taken only by the lanes that leave a BLAS.
template <bool WILD>
MRT_HD bool nf_pop(const TravIn& in, const NfStack& k, Trav& t) {
  if (t.sp == 0) return false;
  t.sp -= 1;
  t.nl = INFINITY;  // a popped node's exit is not kept (LDS: the stack's words are the walk's occupancy limit)
  uint32_t v = k.p[t.sp * k.stride];
  // a marker: kNfRet, or with WILD also kNfWildMark (both bit 31: one test on the common path)
  if (WILD ? (int32_t)v < 0 : v == kNfRet) {
    if (!WILD || v == kNfRet) {
      const bool inst = (t.ret & kRetInstance) != 0;
      t.ret = kNoRet;
      if (inst) {  // a model shares the world ray (and its margin)
        t.r = world_ray(in, t.ray);
        nf_margin(in, t);
      }
      if (t.sp == 0) return false;
      t.sp -= 1;
      v = k.p[t.sp * k.stride];
    }
    if (WILD && v == kNfWildMark) {  // the bottom entry in a scene with a wild tree (walk.h nf_start)
      t.sp = kNfWait;
      t.s1.w = KIND_END;  // never a box (k_trace's box-run ballot)
      return true;
    }
  }
  t.i = v;
  return true;
}
// a waiting lane enters the wild instances' tree: the world ray and its margin
// are in place (every BLAS was left), the stack is empty
MRT_HD void nf_resume_wild(const TravIn& in, Trav& t) {
  t.sp = 0;
  t.i = in.S.nf_wild_root;  // the caller fetches it
}
MRT_HD uint32_t vnf_entry(const DevScene& S, uint32_t base, uint32_t id, uint32_t word) {
  return S.vnf_leaf[2 * (size_t)MRT_IDX(S, S.vnf_base[base] + id, S.n_vnf, 23) + word];
}
// the reference's order of primitive occurrence (prim, ret): {world key, BLAS key}
MRT_HD unsigned long long nf_key(const TravIn& in, uint32_t prim, uint32_t ret) {
  const DevScene& S = in.S;
  const uint32_t kind = prim >> 28, id = prim & 0x0FFFFFFFu;
  if (kind == MRT_REF_SPHERE) return (unsigned long long)vnf_entry(S, VNF_SPHERE, id, 1) << 32;
  const uint32_t k = vnf_entry(S, VNF_TRI, id, 1);
  if (k & kWorldKey) return (unsigned long long)(k & ~kWorldKey) << 32;
  const uint32_t rec = (ret & ~kRetInstance) - 2;  // the NF instance/model record (layout.h)
  const uint32_t cid = in.slots[MRT_IDX(S, rec, S.n_slots, 24)].x;
  const uint32_t wk = vnf_entry(S, (ret & kRetInstance) ? VNF_INST : VNF_MODEL, cid, 1);
  return ((unsigned long long)wk << 32) | k;
}
// does a hit (th, prim, current ret) replace the best so far? (t_max is
// inclusive in the reference: an equal t goes to the later primitive)
MRT_HD bool nf_better(const TravIn& in, const Trav& t, float th, uint32_t prim) {
  if (th < t.best) return true;
  if (!(th == t.best)) return false;
  if (t.prim == kRefNone) return true;
  return nf_key(in, prim, t.ret) > nf_key(in, t.prim, t.hit_ret);
}
// a hit at th (<= the culling bound): the new best, or one of the other hits (t2)
// (selects; the tie's key comparison, which loads, is the only branch)
MRT_HD void nf_hit(const TravIn& in, Trav& t, float th, uint32_t prim) {
  bool better = th < t.best;
  if (th == t.best) better = nf_better(in, t, th, prim);
  t.t2 = vmin1(t.t2, better ? t.best : th);
  t.best = better ? th : t.best;
  t.prim = better ? prim : t.prim;
  t.hit_ret = better ? t.ret : t.hit_ret;
  // a nearer bound: a smaller cap (the line stays valid below it)
  t.nfl.rcb = better ? nf_rho_node(t.nfl, nf_cull(th)) : t.nfl.rcb;
}
// the walk is over: k_trace checks the hit once per loop iteration (nf_finish);
// until then the lane holds an END record, never a box (the box-run ballot)
MRT_HD void nf_over(Trav& t) {
  t.sp = kNfDone;
  t.s1.w = KIND_END;
}

// The reference's box test of reference record `rec` (a box) at t_max = t.
MRT_HD bool ref_box_hits(const TravIn& in, uint32_t rec, const TRay& r, float t) {
  uint4 a, b;
  rec_load2<false>(in, rec, a, b);
  const RecBox x = rec_box(a, b);
  return box_hit_any(x.mn, x.mx, r, in.tmin, t);
}

// The near-first walk is over: does the reference's left-first walk reach
// the winner? The reference enters an ancestor box B of the winner iff
// BoundingBox::hit(B, t_max) holds for its t_max when it gets there, which is
// the smallest t of the hits it accepted BEFORE B — other hits than the
// winner, so at least tau = min(t2, best * (1 + 2^-10)) (t2: the other hits
// this walk met; any hit it did not meet lies beyond the culling margin).
// BoundingBox::hit is monotone in t_max, so B passing at tau suffices; the
// reference's boxes are nested, so the winner's world parent (world ray) and,
// inside a BLAS, its BLAS parent (that space's ray) stand for all of them.
// (Nesting carries over to BoundingBox::hit unless the parent box is flat
// along an axis k and the ray lies in that plane with d_k = 0: 0/0 on both of
// its planes, which min/max pass over, but 0/0 and an infinity on a box above
// with one plane there. Only a sphere can be hit by such a ray; nf_tree.cpp
// builds no trees for a scene with a sphere in a flat reference box.)
// Yes: the ray is done (its record set to END for k_trace's box-run ballot).
// No: the reference's walk from the start (kExactMode).
template <bool COUNT>
MRT_HD void nf_finish(const TravIn& in, Trav& t, LocalCounters& lc) {
  const DevScene& S = in.S;
  bool ok = true;
  const float tau = fminf(t.t2, nf_cull(t.best));
#ifdef MRT_PROBE_NF_NOCHECK  // measurement build only: the winner is not checked (NOT exact)
  if (false) {
#else
  if (t.prim != kRefNone) {
#endif
    const uint32_t kind = t.prim >> 28, id = t.prim & 0x0FFFFFFFu;
    const uint32_t own = vnf_entry(S, kind == MRT_REF_SPHERE ? VNF_SPHERE : VNF_TRI, id, 0);
    if (t.hit_ret == kNoRet) {  // a world object (t.r is the world ray: every BLAS was left)
      if (own != kNoParent) ok = ref_box_hits(in, own, t.r, tau);
    } else {
      const bool inst = (t.hit_ret & kRetInstance) != 0;
      // the NF instance/model record holds its id and its reference world
      // parent (layout.h): one load pair, not id -> vnf_leaf -> parent
      uint4 ra, rb;
      rec_load2<false>(in, (t.hit_ret & ~kRetInstance) - 2, ra, rb);
      const uint32_t cid = ra.x, wpar = rb.x;
      if (wpar != kNoParent) ok = ref_box_hits(in, wpar, t.r, tau);
      if (ok && own != kNoParent) {
        ok = ref_box_hits(in, own, inst ? instance_ray(S, cid, t.r) : t.r, tau);
      }
      if (COUNT) lc.node_visits += 1;
    }
    if (COUNT) lc.node_visits += 1;
  }
  if (ok) {
    t.done = true;
    t.s1.w = KIND_END;  // a done lane holds an END record (k_trace's box-run ballot)
    return;
  }
  if (COUNT) lc.vnf_fallbacks++;
  t.sp = kExactMode;  // the reference's walk (the caller fetches t.i)
  t.i = in.world_begin;
  t.ret = kNoRet;
  t.best = in.tmax0;
  t.prim = kRefNone;
  t.hit_ret = kNoRet;
}

// Both children's boxes of an NF node (layout.h NF NODE) against [tmin,
// tmax], each thickened by rho = nfm (nf_bound.h): hit[c] unless the box is
// certainly missed, ent[c] its entry t. Fast rays: plane t = q * (2^e * y) +
// (o * y - oy) -/+ rho * y — 2^e * y is exact, so the error against (plane -/+
// rho - o_ray) / d adds the node's |o * y - oy -/+ rho * y| term to the early
// decision's margin (box_hit_any; rho carries a 2^-20 excess for the
// rounding of rho * y against rho / d) — and only a certain miss counts as
// one: the walk's boxes may be loose (its hits are checked against the
// reference tree), never tight. Other rays: the exact test on the decoded
// planes moved out by rho and widened by an ulp. A child whose force bit is
// set (kNfForceL/R: a wild instance below, nf_bound.h NfWild) is never culled
// here; the wild instance's own leaf test decides (trav_prim_index_nf).
MRT_HD void nf_node_test(const uint4& s0, const uint4& s1, const TRay& r, float tmin, float tmax, float nfm, bool hit[2],
                          float ent[2], float ex[2]) {
  const V3 o{u2f(s0.x), u2f(s0.y), u2f(s0.z)};
  const V3 sc{u2f((s0.w & 0xFFu) << 23), u2f(((s0.w >> 8) & 0xFFu) << 23), u2f(((s0.w >> 16) & 0xFFu) << 23)};
  const uint32_t qw[3] = {s1.x, s1.y, s1.z};
  auto q = [&](int j) { return (float)((qw[j >> 2] >> (8 * (j & 3))) & 0xFFu); };  // v_cvt_f32_ubyteN
  // both paths leave floats only (entry, entry - exit, margin, exit bound):
  // the hit flags are formed after the merge, so no lane mask is carried
  // across it in vector registers
  float t0[2], dt[2], m[2], xb[2];
  if (tray_fast(r)) {
    const float ax = sc.x * r.yx, ay = sc.y * r.yy, az = sc.z * r.yz;
    const float bx = fmaf(o.x, r.yx, -r.oyx), by = fmaf(o.y, r.yy, -r.oyy), bz = fmaf(o.z, r.yz, -r.oyz);
    const float lbx = fmaf(-nfm, r.yx, bx), lby = fmaf(-nfm, r.yy, by), lbz = fmaf(-nfm, r.yz, bz);
    const float hbx = fmaf(nfm, r.yx, bx), hby = fmaf(nfm, r.yy, by), hbz = fmaf(nfm, r.yz, bz);
    const float mabs = fmaf(vmax3ab(lbx, lby, vmax3ab(lbz, hbx, vmax3ab(hby, hbz, 0.0f))), 0x1p-20f, fabsf(r.om));
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int b = 6 * c;
      const float lx = fmaf(q(b), ax, lbx), ly = fmaf(q(b + 1), ay, lby), lz = fmaf(q(b + 2), az, lbz);
      const float hx = fmaf(q(b + 3), ax, hbx), hy = fmaf(q(b + 4), ay, hby), hz = fmaf(q(b + 5), az, hbz);
      t0[c] = vmax3(vmin1(lx, hx), vmin1(ly, hy), vmax1(vmin1(lz, hz), tmin));
      const float t1 = vmin3(vmax1(lx, hx), vmax1(ly, hy), vmin1(vmax1(lz, hz), tmax));
      m[c] = fmaf(fabsf(t0[c]) + fabsf(t1), 0x1p-19f, mabs);
      dt[c] = t0[c] - t1;
      // every hit in the thickened box has t <= this (m covers t1's error and this rounding)
      xb[c] = fmaf(m[c], 2.0f, t1);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int b = 6 * c;
      auto lo = [&](float qq, float s, float org) {
        const float p = fmaf(qq, s, org) - nfm;
        return p - fmaf(fabsf(p), 0x1p-23f, 0x1p-140f);
      };
      auto hi = [&](float qq, float s, float org) {
        const float p = fmaf(qq, s, org) + nfm;
        return p + fmaf(fabsf(p), 0x1p-23f, 0x1p-140f);
      };
      const V3 mn{lo(q(b), sc.x, o.x), lo(q(b + 1), sc.y, o.y), lo(q(b + 2), sc.z, o.z)};
      const V3 mx{hi(q(b + 3), sc.x, o.x), hi(q(b + 4), sc.y, o.y), hi(q(b + 5), sc.z, o.z)};
      const V3 a = (mn - r.o) / r.d, bb = (mx - r.o) / r.d;  // IEEE quotients (the planes may lie outside the qfast domain)
      t0[c] = vmax3(vmin1(a.x, bb.x), vmin1(a.y, bb.y), vmax1(vmin1(a.z, bb.z), tmin));
      const float t1 = vmin3(vmax1(a.x, bb.x), vmax1(a.y, bb.y), vmin1(vmax1(a.z, bb.z), tmax));
      dt[c] = t0[c] - t1;  // > 0 exactly when t1 < t0 (+-inf pairs: NaN, a hit as !(t1 < t0))
      m[c] = 0.0f;
      xb[c] = INFINITY;  // no exit bound from the exact quotients
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const bool force = (s1.w & (kNfForceL << c)) != 0;
    hit[c] = !(dt[c] > m[c]) || force;
    ent[c] = t0[c];
    // a forced child holds a wild instance, whose hits the world margin does
    // not place inside the box: no exit bound below it
    ex[c] = force ? INFINITY : xb[c];
  }
}

// does any lane of the wave hold p? (a host "wave" is one lane)
MRT_HD bool wave_any(bool p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_ballot_w64(p) != 0;
#else
  return p;
#endif
}

// The current record is an NF node: both children's boxes tested (culling at
// best * (1 + 2^-10)); both hit: the nearer next, the other pushed; one: that
// one; none: the stack's next.
template <bool COUNT, bool WILD>
MRT_HD void trav_box_index_nf(const TravIn& in, const NfStack& k, Trav& t, LocalCounters& lc) {
  if (COUNT) lc.node_visits += 2;
  bool h[2];
  float e[2], x[2];
  // the hits this node must keep have t <= min(cull(best), nl)
  const float cb = nf_cull(t.best);
#ifdef MRT_PROBE_NF_ZERO_RHO  // measurement build only: no rounding margin (NOT exact)
  const float rho = 0.0f;
#elif defined(MRT_PROBE_NF_NOCONE)  // measurement build only: the ray's generic term everywhere (exact, looser)
  const float rho = nf_rho_node(t.nfl, fminf(cb, t.nl));
#else
  // the node's normal cone narrows the generic-triangle term (nf_bound.h
  // nf_cone_rg); scenes without generic triangles (kc == 0) skip it
  // (the cones only while some lane's worst-case generic term is worth it:
  // a wave-uniform choice, either rho is valid)
  const float tn = vmin1(cb, t.nl);
  float rho = nf_rho_node(t.nfl, tn);
  if (in.S.nfb.kc > 0.0f && wave_any(t.nfl.rg * tn > in.S.nfb.kcmin))
    rho = nf_rho_cone(t.nfl, tn, t.s0.x, t.s0.y, t.s0.z, t.s0.w, t.r.d);
#endif
  nf_node_test(t.s0, t.s1, t.r, in.tmin, cb, rho, h, e, x);
  const uint32_t base = t.s1.w & kNfIdx, right = base + 2u + ((t.s0.w >> 24) & 1u);  // lsz - 2 in bit 24 (layout.h)
  // selects for the next record and its exit bound, the push and the pop as
  // the only branches (the left child when it is hit and nearer, or alone)
  const bool left = h[0] && (!h[1] || !(e[1] < e[0]));
  t.i = left ? base : right;
  t.nl = left ? x[0] : x[1];
  if (h[0] && h[1]) nf_push(k, t, left ? right : base);
  if (!(h[0] || h[1]) && !nf_pop<WILD>(in, k, t)) nf_over(t);
}

// A wild instance's leaf record (slot0.w: its WILD entry, layout.h): does the
// world ray meet its world box thickened by its own margin at [tmin,
// cull(best)]? (nf_bound.h NfWild; the nodes above it never cull it)
MRT_HD bool nf_wild_enter(const TravIn& in, const Trav& t, uint32_t at) {
  const uint4 a = rec_load1<false>(in, at), b = rec_load1<false>(in, at + 1), c = rec_load1<false>(in, at + 2),
              e = rec_load1<false>(in, at + 3);
  const NfWild x{{u2f(a.x), u2f(a.y), u2f(a.z)}, {u2f(a.w), u2f(b.x), u2f(b.y)}, u2f(b.z), u2f(b.w), u2f(c.x), u2f(c.y),
                 {u2f(c.z), u2f(c.w), u2f(e.x)}, u2f(e.y)};
  return nf_wild_hit(x, t.r.o, t.r.d, t.r.a.b, in.tmin, nf_cull(t.best));
}

// The current record is an NF leaf's primitive, instance or model.
template <bool COUNT, uint32_t ALPHA, bool WILD>
MRT_HD void trav_prim_index_nf(const TravIn& in, const NfStack& k, Trav& t, LocalCounters& lc) {
  const DevScene& S = in.S;
  const uint4 s0 = t.s0, s1 = t.s1;
  const uint32_t kind = s1.w;
  uint32_t next;
  if (kind == KIND_TRI) {
    if (COUNT) lc.triangle_tests++;
    const uint4 s2 = rec_load1<false>(in, t.i + 2);
    const RecTri v = rec_tri(s0, s1, s2);
    float th;
    // tested up to the culling bound: hits beyond `best` are recorded in t2
    if (tri_hit_nb(v.a, v.ab, v.ac, t.r.o, t.r.d, in.tmin, nf_cull(t.best), th)) {
      const uint32_t id = s1.z & kTriIdMask;
      if (!ALPHA || !(s1.z & kTriAlpha) || tri_alpha_pass<false, ALPHA == 2>(S, id, t.r.o, t.r.d, th, t.rng, lc))
        nf_hit(in, t, th, make_ref(MRT_REF_TRIANGLE, id));
    }
    next = s2.w;
  } else if (kind == KIND_SPHERE) {
    if (COUNT) lc.sphere_tests++;
    float th;
    if (sphere_hit(V3{u2f(s0.x), u2f(s0.y), u2f(s0.z)}, u2f(s0.w), t.r.o, t.r.d, t.r.a, in.tmin, nf_cull(t.best), th))
      nf_hit(in, t, th, make_ref(MRT_REF_SPHERE, s1.x));
    next = s1.y;
  } else if (kind == KIND_INST && s0.w != 0 && !nf_wild_enter(in, t, s0.w)) {
    next = s0.z;  // a wild instance the ray passes by (its own box and margin)
  } else {  // KIND_INST / KIND_MODEL: enter its BLAS, come back to the leaf's next record
    if (s0.z != kNfPop) nf_push(k, t, s0.z);
    nf_push(k, t, kNfRet);
    if (kind == KIND_INST) {
      if (COUNT) lc.instance_entries++;
      t.r = instance_ray(S, s0.x, t.r);
      t.ret = (t.i + 2) | kRetInstance;
      nf_margin(in, t);  // the object space's margin
    } else {
      if (COUNT) lc.model_entries++;
      t.ret = t.i + 2;
    }
    t.i = s0.y;
    return;
  }
  t.i = next;
  if (next == kNfPop && !nf_pop<WILD>(in, k, t)) nf_over(t);
}

// ---- the step a lane takes (k_trace; the host's replay in tools/slab_check.cpp) ----
// NF: the kernel walks near-first, and only a lane that fell back (sp ==
// kExactMode) takes the reference's steps; else every lane does.
template <bool COUNT, bool NF, bool WILD>
MRT_HD void trav_box_index_either(const TravIn& in, const NfStack& k, Trav& t, LocalCounters& lc) {
  if (NF && t.sp != kExactMode)
    trav_box_index_nf<COUNT, WILD>(in, k, t, lc);
  else
    trav_box_index<COUNT>(in, t, lc);
}
template <bool COUNT, uint32_t ALPHA, bool RNG, bool LDS, bool VBLAS, bool NF, bool WILD>
MRT_HD void trav_prim_index_either(const TravIn& in, const NfStack& k, Trav& t, LocalCounters& lc) {
  if (NF && t.sp != kExactMode)
    trav_prim_index_nf<COUNT, ALPHA, WILD>(in, k, t, lc);
  else
    trav_prim_index<COUNT, ALPHA, RNG, LDS, VBLAS>(in, t, lc);
}
// the lane may fetch its next record: it is neither done nor waiting
template <bool NF, bool WILD>
MRT_HD bool trav_may_fetch(const Trav& t) { return !t.done && (!NF || !nf_parked<WILD>(t)); }

}  // namespace mrt
