// records.h — the host's one reading of the record table in layout.h: every
// word of a record that host code reads, writes or patches has its number
// here and nowhere else (upload.cpp, nf_tree.cpp and the host tools under
// tools/ go through these functions). The device walk (walk.h, walk_nf.h) is
// the other reader: it takes records apart as s0 / s1 / s2 components.
// Host-only: no .hip file and no header a .hip file includes may include this.
//
// w: the slot array (4 words per slot); i: a record's first slot. A record's
// words below are numbered from its first slot (rec[7] is slot1.w, the kind).
#pragma once
#include <string.h>

#include <vector>

#include "layout.h"

namespace mrt {
namespace rec {

inline const uint32_t* at(const uint32_t* w, uint32_t i) { return w + 4 * (size_t)i; }
inline uint32_t* at(uint32_t* w, uint32_t i) { return w + 4 * (size_t)i; }
inline float f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
inline uint32_t u32(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
// words [k, k + 3) of record i as floats
inline void f32x3(const uint32_t* w, uint32_t i, int k, float v[3]) { memcpy(v, at(w, i) + k, 12); }

// ---- every record ----
inline uint32_t kind(const uint32_t* w, uint32_t i) { return at(w, i)[7]; }  // a box: kBoxFlag | hit
inline bool is_box(const uint32_t* w, uint32_t i) { return (kind(w, i) & kBoxFlag) != 0; }
inline uint32_t n_slots(const uint32_t* w, uint32_t i) { return kind(w, i) == KIND_TRI ? 3u : 2u; }
inline void copy(uint32_t* dst, const uint32_t* w, uint32_t i) { memcpy(dst, at(w, i), 16 * (size_t)n_slots(w, i)); }

// ---- reference stream: BOX ----
inline uint32_t box_hit(const uint32_t* w, uint32_t i) { return at(w, i)[7] & ~kBoxFlag; }
inline uint32_t box_skip(const uint32_t* w, uint32_t i) { return at(w, i)[6]; }
inline void box_bounds(const uint32_t* w, uint32_t i, float mn[3], float mx[3]) { f32x3(w, i, 0, mn), f32x3(w, i, 3, mx); }
inline void set_box_skip(uint32_t* w, uint32_t i, uint32_t skip) { at(w, i)[6] = skip; }

// ---- SPHERE, and a VOLUME over its own sphere ----
inline void sphere_center(const uint32_t* w, uint32_t i, float c[3]) { f32x3(w, i, 0, c); }
inline float sphere_radius(const uint32_t* w, uint32_t i) { return f32(at(w, i)[3]); }
inline uint32_t sphere_id(const uint32_t* w, uint32_t i) { return at(w, i)[4]; }

// ---- TRI ----
inline void tri_a(const uint32_t* w, uint32_t i, float v[3]) { f32x3(w, i, 0, v); }
inline void tri_ab(const uint32_t* w, uint32_t i, float v[3]) { f32x3(w, i, 3, v); }
inline void tri_ac(const uint32_t* w, uint32_t i, float v[3]) { f32x3(w, i, 8, v); }
inline uint32_t tri_id(const uint32_t* w, uint32_t i) { return at(w, i)[6] & kTriIdMask; }

// ---- INST / MODEL (their id is word 0 in the NF trees' leaves too) ----
inline uint32_t object_id(const uint32_t* w, uint32_t i) { return at(w, i)[0]; }
inline uint32_t blas_begin(const uint32_t* w, uint32_t i) { return at(w, i)[1]; }
inline void set_blas_range(uint32_t* w, uint32_t i, uint32_t begin, uint32_t end) { at(w, i)[1] = begin, at(w, i)[2] = end; }

// ---- VOLUME ----
inline uint32_t volume_target(const uint32_t* w, uint32_t i) { return at(w, i)[6]; }  // 0, kVolInstance, kVolModel
inline void set_volume_blas(uint32_t* w, uint32_t i, uint32_t begin) { at(w, i)[0] = begin; }  // of an instance / model target

// ---- successors ----
// the record the walk reaches after primitive i; an instance or model returns to the record after it
inline uint32_t next(const uint32_t* w, uint32_t i) {
  const uint32_t k = kind(w, i);
  return k == KIND_INST || k == KIND_MODEL ? i + 2 : at(w, i)[k == KIND_TRI ? 11 : 5];
}
// record i's successor at its own level: past a box's subtree, else next
inline uint32_t successor(const uint32_t* w, uint32_t i) { return is_box(w, i) ? box_skip(w, i) : next(w, i); }
// f(record) for the items of a level: from `first` along successors until
// `end` (a box's skip, for its children; ~0u: none) or the region's END record
template <class F>
inline void for_each_in_level(const uint32_t* w, uint32_t first, uint32_t end, F f) {
  for (uint32_t c = first; c != end && kind(w, c) != KIND_END; c = successor(w, c)) f(c);
}
// the same items as a list, and those of box i (its children, in order)
inline void level(const uint32_t* w, uint32_t first, uint32_t end, std::vector<uint32_t>& out) {
  out.clear();
  for_each_in_level(w, first, end, [&](uint32_t c) { out.push_back(c); });
}
inline void box_children(const uint32_t* w, uint32_t i, std::vector<uint32_t>& out) { level(w, box_hit(w, i), box_skip(w, i), out); }

// ---- links: the words of a reference-stream record that name another record ----
enum LinkKind { kLinkSuccessor, kLinkBlasBegin, kLinkBlasEnd };
// f(uint32_t& index, LinkKind) for each of them; a box's hit keeps its flag bit
template <class F>
inline void for_each_link(uint32_t* rec, F f) {
  const uint32_t k = rec[7];
  if (k & kBoxFlag) {
    uint32_t hit = k & ~kBoxFlag;
    f(rec[6], kLinkSuccessor);
    f(hit, kLinkSuccessor);
    rec[7] = kBoxFlag | hit;
  } else if (k == KIND_TRI) {
    f(rec[11], kLinkSuccessor);
  } else if (k == KIND_SPHERE || k == KIND_VOLUME) {
    f(rec[5], kLinkSuccessor);
    if (k == KIND_VOLUME && rec[6]) f(rec[0], kLinkBlasBegin);  // its target's BLAS
  } else if (k == KIND_INST || k == KIND_MODEL) {
    f(rec[1], kLinkBlasBegin);
    f(rec[2], kLinkBlasEnd);
  }
}

// ---- a leaf object's verification slot (layout.h vnf_leaf) ----
inline uint32_t vnf_slot(const uint32_t* w, uint32_t i, const uint32_t vnf_base[4]) {
  switch (kind(w, i)) {
    case KIND_SPHERE: return vnf_base[VNF_SPHERE] + sphere_id(w, i);
    case KIND_TRI: return vnf_base[VNF_TRI] + tri_id(w, i);
    case KIND_INST: return vnf_base[VNF_INST] + object_id(w, i);
    default: return vnf_base[VNF_MODEL] + object_id(w, i);
  }
}

// ---- NF NODE ----
inline uint32_t nf_children(const uint32_t* w, uint32_t i) { return at(w, i)[7] & kNfIdx; }   // the left child's record
inline uint32_t nf_left_slots(const uint32_t* w, uint32_t i) { return 2u + ((at(w, i)[3] >> 24) & 1u); }
// the node's frame: origin bits and the word {ex, ey, ez, lsz | cone code} (walk_nf.h takes them as s0)
struct NfFrame {
  uint32_t ox, oy, oz, ew;
};
inline NfFrame nf_frame(const uint32_t* w, uint32_t i) { return {at(w, i)[0], at(w, i)[1], at(w, i)[2], at(w, i)[3]}; }
// fills node i: frame origin o, exponents ew (8 bits per axis), the children's
// quantized planes q, the left child's size, the cone code, the force flags,
// the children's first record
inline void put_nf_node(uint32_t* w, uint32_t i, const uint32_t o[3], uint32_t ew, const uint32_t q[3], uint32_t left_slots,
                        uint32_t cone_code, uint32_t force, uint32_t children) {
  uint32_t* r = at(w, i);
  r[0] = o[0], r[1] = o[1], r[2] = o[2], r[3] = ew | (left_slots - 2) << 24 | cone_code << 25;
  r[4] = q[0], r[5] = q[1], r[6] = q[2], r[7] = kBoxFlag | force | children;
}

// ---- NF leaves: SPHERE / TRI as in the reference stream; INST / MODEL ----
inline uint32_t nf_next_word(const uint32_t* w, uint32_t i) {
  const uint32_t k = kind(w, i);
  return k == KIND_TRI ? 11u : k == KIND_SPHERE ? 5u : 2u;
}
inline uint32_t nf_next(const uint32_t* w, uint32_t i) { return at(w, i)[nf_next_word(w, i)]; }  // kNfPop: the leaf's last
inline void set_nf_next(uint32_t* w, uint32_t i, uint32_t n) { at(w, i)[nf_next_word(w, i)] = n; }
inline uint32_t nf_blas_root(const uint32_t* w, uint32_t i) { return at(w, i)[1]; }
inline uint32_t nf_wild(const uint32_t* w, uint32_t i) { return at(w, i)[3]; }  // its WILD entry's first slot, 0: none
inline void set_nf_blas_root(uint32_t* w, uint32_t i, uint32_t root) { at(w, i)[1] = root; }
inline void set_nf_wild(uint32_t* w, uint32_t i, uint32_t entry) { at(w, i)[3] = entry; }
inline void set_nf_parent(uint32_t* w, uint32_t i, uint32_t parent) { at(w, i)[4] = parent; }
// WILD entry (nf_bound.h NfWild), 4 slots: the struct's 14 floats, then zeros
inline NfWild nf_wild_entry(const uint32_t* w, uint32_t i) {
  NfWild e;
  memcpy(&e, at(w, i), sizeof e);
  return e;
}

// ---- writers: each appends one record to the slot vector and returns its first slot ----
inline uint32_t grow(std::vector<uint32_t>& w, uint32_t slots) {  // zeroed slots
  const uint32_t i = (uint32_t)(w.size() / 4);
  w.resize(w.size() + 4 * (size_t)slots, 0u);
  return i;
}
inline uint32_t put(std::vector<uint32_t>& w, const uint32_t (&r)[8]) {
  const uint32_t i = (uint32_t)(w.size() / 4);
  w.insert(w.end(), r, r + 8);
  return i;
}
// hit: the record after it (its first child); skip: set_box_skip, once its subtree is written
inline uint32_t put_box(std::vector<uint32_t>& w, const float mn[3], const float mx[3]) {
  const uint32_t i = (uint32_t)(w.size() / 4);
  return put(w, {u32(mn[0]), u32(mn[1]), u32(mn[2]), u32(mx[0]), u32(mx[1]), u32(mx[2]), 0, kBoxFlag | (i + 2)});
}
// sphere, triangle and volumes: next = the record after it
inline uint32_t put_sphere(std::vector<uint32_t>& w, const float c[3], float r, uint32_t id, uint32_t k = KIND_SPHERE) {
  const uint32_t i = (uint32_t)(w.size() / 4);
  return put(w, {u32(c[0]), u32(c[1]), u32(c[2]), u32(r), id, i + 2, 0, k});
}
inline uint32_t put_volume_sphere(std::vector<uint32_t>& w, const float c[3], float r, uint32_t id) {
  return put_sphere(w, c, r, id, KIND_VOLUME);
}
// target: kVolInstance / kVolModel and the instance's / model's id; its BLAS: set_volume_blas
inline uint32_t put_volume_blas(std::vector<uint32_t>& w, uint32_t id, uint32_t target, uint32_t target_id) {
  const uint32_t i = (uint32_t)(w.size() / 4);
  return put(w, {0, target_id, 0, 0, id, i + 2, target, KIND_VOLUME});
}
// id_alpha: the triangle's id, kTriAlpha set when it is alpha-tested
inline uint32_t put_tri(std::vector<uint32_t>& w, const float a[3], const float ab[3], const float ac[3], uint32_t id_alpha) {
  const uint32_t i = put(w, {u32(a[0]), u32(a[1]), u32(a[2]), u32(ab[0]), u32(ab[1]), u32(ab[2]), id_alpha, KIND_TRI});
  const uint32_t s2[4] = {u32(ac[0]), u32(ac[1]), u32(ac[2]), i + 3};
  w.insert(w.end(), s2, s2 + 4);
  return i;
}
// k: KIND_INST or KIND_MODEL; its BLAS range: set_blas_range
inline uint32_t put_inst_or_model(std::vector<uint32_t>& w, uint32_t k, uint32_t id) { return put(w, {id, 0, 0, 0, 0, 0, 0, k}); }
inline uint32_t put_end(std::vector<uint32_t>& w) { return put(w, {0, 0, 0, 0, 0, 0, 0, KIND_END}); }
inline uint32_t put_nf_wild(std::vector<uint32_t>& w, const NfWild& e) {
  static_assert(sizeof(NfWild) == 56, "a WILD entry is NfWild's 14 floats and two zero words");
  const uint32_t i = grow(w, 4);
  memcpy(at(w.data(), i), &e, sizeof e);
  return i;
}

}  // namespace rec
}  // namespace mrt
