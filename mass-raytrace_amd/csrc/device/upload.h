// upload.h — mrt_scene_desc (reference tree) -> HBM layout (layout.h).
#pragma once
#include <string>
#include <vector>

#include "../../../include/massrt.h"
#include "layout.h"

namespace mrt {

// A BLAS region of the stream: records [begin, end) plus the END record at end.
struct BlasRegion {
  uint32_t begin, end, refs;  // refs: instance/model records entering it
  bool model;                 // entered by a model (world space) at least once
};

struct HostScene {
  std::vector<uint32_t> slots;  // 4 words per slot
  std::vector<uint32_t> rec_starts;  // first slot of every record, ascending (padding slots are not records)
  uint32_t world_begin = 0, world_end = 0;
  std::vector<float> inst_inv, inst_fwd;
  std::vector<uint32_t> inst_mat, model_mat;
  std::vector<float> sph;
  std::vector<uint32_t> sph_mat;
  std::vector<float> tri_shade;
  std::vector<float> eve;     // EveMaterial records (layout.h kEveQuads)
  std::vector<float> tri_tb;  // tangent / bitangent per triangle; empty unless the scene has an Eve material
  std::vector<GpuMaterial> materials;
  std::vector<GpuTexture> textures;
  std::vector<uint32_t> texels;
  uint32_t fast_ok = 1;   // every box coordinate in {0} U [2^-40, 2^28]: the exact slab test may use qfast
  uint32_t early_ok = 1;  // every box coordinate finite and within 2^28: the early slab decision applies
  bool has_alpha = false;  // some triangle carries TRI_FLAG_ALPHA
  bool trav_rng = false;   // the traversal draws random numbers (Volume, Mix alpha tests)
  bool vol_blas = false;   // some volume's target is an instance or a model (walk.h volume_hit_blas)
  std::vector<float> vol_nid;
  std::vector<uint32_t> vol_mat;
  // Volume draws f = m * 2^-23 (m < 2^23, mrt_rng.h) and takes f.ln()
  // (geom.rs:640): the device looks up the host libm logf of every such f
  // instead of computing it, so the distance is the reference's to the bit
  // (32 MiB, built only when the scene has volumes).
  std::vector<float> ln_table;
  std::vector<GpuSurfOp> surf_ops;
  uint32_t bg_kind = 0;
  float bg_color[4] = {0, 0, 0, 0};
  std::vector<GpuSurfRef> bg_faces;  // SkySphere 1, CubeMap 6
  float bg_m[16] = {0};
  std::vector<BlasRegion> blas_regions;
  // LDS treelet (build_treelet): image (4 words per slot), rewritten stream, world entry
  std::vector<uint32_t> tlet, slots_tl;
  uint32_t tl_world_begin = 0, tl_boxes = 0;
  // statistics
  uint32_t n_box_records = 0, n_prim_records = 0, max_depth = 0;
  // verified near-first trees (nf_tree.cpp): appended to `slots` after the
  // reference stream (not in rec_starts: the treelet and relayout never see them)
  bool nf_ok = false;
  uint32_t nf_world = 0, nf_boxes = 0, nf_stack_need = 0, nf_first_slot = 0;
  std::vector<uint32_t> vnf_leaf;  // {parent, key} pairs
  uint32_t vnf_base[4] = {0, 0, 0, 0};
  std::string nf_note;  // why a scene has no NF trees
  NfBound nfb{};         // the walk's rounding margins (nf_bound.h, nf_tree.cpp)
  uint32_t nf_wild = 0;  // instances the world margin does not cover: never culled
  uint32_t nf_wild_root = 0;  // their own tree's root record, walked after the world tree (0: none, or it is nf_world)
  uint32_t nf_cones = 0;  // NF nodes carrying a normal cone (nf_bound.h nf_cone_rg)
  // triangles under the generic bound (nf_tree.cpp tri_bound): those off every coordinate plane, and those on
  // one that left the coordinate-plane bound by one of its exits (degenerate, beta < 0.5, kappa too large)
  uint32_t nf_generic = 0, nf_generic_planar = 0;
  // tools/slab_check: set before building to keep every leaf object's NF box
  // (6 floats per vnf_leaf slot: mn xyz, mx xyz) and which instances are wild
  bool keep_nf_boxes = false;
  // which NF trees to build (set before build_host_scene; the option
  // "traversal" at upload): kNfBuildAuto builds them unless the per-scene
  // rule would walk the reference's way anyway (a generic-triangle term, or a
  // big instanced world), kNfBuildNever skips them, kNfBuildAlways builds them
  int nf_build = 2;
  std::vector<float> nf_leaf_box;
  std::vector<uint8_t> nf_inst_wild;
};

enum { kNfBuildNever = 0, kNfBuildAlways = 1, kNfBuildAuto = 2 };

// The scene's device arrays, listed once, in the order the upload places
// them: f(DevScene member, host data, bytes, flags) per array. host_dev_scene
// and the upload (api.hip mrt_upload_scene_targets) both set the DevScene's
// pointers from this list, so a new array is one entry here plus its
// HostScene and DevScene fields.
enum : unsigned {
  kArrNullIfEmpty = 1,  // the kernels test the pointer: null when the array is empty
  kArrDeviceOnly = 2,   // the LDS treelet's arrays: not part of host_dev_scene
};
template <typename F>
void for_each_scene_array(const HostScene& s, F&& f) {
  auto vec = [&](auto field, const auto& v, unsigned flags = 0) { f(field, v.data(), v.size() * sizeof(v[0]), flags); };
  vec(&DevScene::slots, s.slots);
  vec(&DevScene::slots_tl, s.slots_tl, kArrDeviceOnly);
  vec(&DevScene::tlet, s.tlet, kArrDeviceOnly);
  vec(&DevScene::inst_inv, s.inst_inv);
  vec(&DevScene::inst_fwd, s.inst_fwd);
  vec(&DevScene::inst_mat, s.inst_mat);
  vec(&DevScene::model_mat, s.model_mat);
  vec(&DevScene::sph, s.sph);
  vec(&DevScene::sph_mat, s.sph_mat);
  vec(&DevScene::tri_shade, s.tri_shade);
  vec(&DevScene::materials, s.materials);
  vec(&DevScene::textures, s.textures);
  vec(&DevScene::texels, s.texels);
  vec(&DevScene::vol_nid, s.vol_nid);
  vec(&DevScene::vol_mat, s.vol_mat);
  vec(&DevScene::ln_table, s.ln_table, kArrNullIfEmpty);
  vec(&DevScene::surf_ops, s.surf_ops);
  vec(&DevScene::bg_faces, s.bg_faces);
  f(&DevScene::bg_m, &s.bg_m[0], sizeof(s.bg_m), 0u);
  vec(&DevScene::vnf_leaf, s.vnf_leaf);
  vec(&DevScene::eve, s.eve);
  vec(&DevScene::tri_tb, s.tri_tb, kArrNullIfEmpty);
}

// Where the upload puts the arrays: 256-byte-aligned sections, in the list's
// order, inside one device allocation of total + 256 bytes.
struct ScenePlan {
  std::vector<size_t> off;  // per list entry
  size_t total = 0;         // what mrt_scene_device_bytes reports
};
inline ScenePlan plan_scene(const HostScene& s) {
  ScenePlan p;
  for_each_scene_array(s, [&](auto, const void*, size_t bytes, unsigned) {
    p.off.push_back(p.total);
    p.total += (bytes + 255) & ~(size_t)255;
  });
  return p;
}

// The kernel-visible scene over the HostScene's own vectors (no treelet, no
// debug record): what the walk's host callers pass to the device headers'
// functions (tools/slab_check.cpp; valid while `s` lives unchanged), and what
// mrt_upload_scene starts from before it points the arrays at the device copies.
inline DevScene host_dev_scene(const HostScene& s) {
  DevScene S{};
  for_each_scene_array(s, [&](auto field, auto* data, size_t bytes, unsigned flags) {
    if (!(flags & kArrDeviceOnly)) S.*field = bytes || !(flags & kArrNullIfEmpty) ? data : nullptr;
  });
  S.world_begin = s.world_begin;
  S.world_end = s.world_end;
  S.fast_ok = (s.fast_ok ? 1u : 0u) | (s.early_ok ? 2u : 0u);
  S.n_slots = (uint32_t)(s.slots.size() / 4);
  S.n_tris = (uint32_t)(s.tri_shade.size() / (kTriShadeQuads * 4));
  S.n_sph = (uint32_t)s.sph_mat.size();
  S.n_inst = (uint32_t)s.inst_mat.size();
  S.n_models = (uint32_t)s.model_mat.size();
  S.n_materials = (uint32_t)s.materials.size();
  S.n_textures = (uint32_t)s.textures.size();
  S.n_texels = (uint32_t)s.texels.size();
  S.n_vol = (uint32_t)s.vol_nid.size();
  S.n_surf_ops = (uint32_t)s.surf_ops.size();
  S.bg_kind = s.bg_kind;
  for (int k = 0; k < 4; ++k) S.bg_color[k] = s.bg_color[k];
  S.nf_ok = s.nf_ok ? 1u : 0u;
  S.nf_world = s.nf_world;
  S.nf_wild_root = s.nf_ok ? s.nf_wild_root : 0u;
  for (int k = 0; k < 4; ++k) S.vnf_base[k] = s.vnf_base[k];
  S.n_vnf = (uint32_t)(s.vnf_leaf.size() / 2);
  S.nfb = s.nfb;
  S.n_eve = (uint32_t)(s.eve.size() / (kEveQuads * 4));
  return S;
}

// Builds the verified near-first trees of a linearised scene (after
// build_host_scene; layout.h). A scene whose traversal draws random numbers,
// or whose trees would need more than kNfStack stack entries, gets none
// (nf_ok false, nf_note says why). Returns false only on an internal error.
bool build_nf_trees(const mrt_scene_desc& d, HostScene& s, std::string& err);

// Validates the description and linearises it. Returns false with `err` set.
// sibling_layout=false keeps every region in plain preorder (the layout
// before round 2; tools/slab_check.cpp runs the walk over both: they walk alike)
// ext: the tables beside the description (mrt_upload_scene_ext); null: none.
// targets: the volumes whose boundary is an instance or a model
// (mrt_upload_scene_targets).
bool build_host_scene(const mrt_scene_desc& d, HostScene& out, std::string& err, bool sibling_layout = true,
                      const mrt_scene_ext* ext = nullptr, const mrt_volume_target* targets = nullptr,
                      uint32_t n_targets = 0);

// Chooses the records copied into LDS by every k_trace workgroup (at most
// `budget` 16-byte slots): the whole stream when it fits; else the small BLAS
// regions whole (most referenced first, within budget/4) and then boxes of the
// world tree and of model BLAS in decreasing surface area — a rooted treelet.
// Fills s.tlet (the LDS image), s.slots_tl (the stream with its indices
// rewritten to reach the copies) and s.tl_world_begin. budget 0: no treelet.
void build_treelet(HostScene& s, uint32_t budget);

}  // namespace mrt
