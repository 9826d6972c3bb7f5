// options.h — the context options (mrt_set_option / mrt_get_option, massrt.h)
// and everything derived from them. Plain C++, no HIP: the per-scene rules are a
// pure function of the options and a few scene facts (tests/test_options.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "../../../include/massrt.h"

namespace mrt {

// Path pools on their own streams, at most (option "queues").
constexpr int kMaxQueues = 4;

// The tuning knobs of the loop, set by the caller per context — never read
// from the process environment. -1 (where allowed) = the per-scene rule
// (derive_tuning). Measurements behind each default: DESIGN.md §4.
enum OptId {
  OPT_QUEUES,            // path pools on their own streams (2: one's tail overlaps the other's kernels)
  OPT_POOL_PATHS,        // live paths at most over all queues (384M: 66 GiB)
  OPT_RESULTS_LOG2,      // samples per results slab at most, log2 (31: a 1080p x 1024-spp frame in one chunk)
  OPT_FINISH_PATHS,      // drain hand-off threshold (fused adopt-mode launch); 0 = never
  OPT_FINISH_GRID_DIV,   // the hand-off launch takes 1/div of its occupancy grid
  OPT_TRACE_REFILL,      // k_trace: refill a wave once this many lanes are idle (-1: 32)
  OPT_TRACE_BOX_MIN,     // k_trace: box run while this many lanes are at a box (-1: 16 instanced / 32 big / 24)
  OPT_TRACE_CHUNK,       // k_trace: rays per work grab (-1: 128 big or instanced / 512)
  OPT_TRACE_PRIM_BATCH,  // k_trace: primitive step once this many lanes wait at one
  OPT_TRACE_WGS_PER_CU,  // persistent grids: workgroups per CU (0: occupancy, 3/4 of it beside other queues)
  OPT_SHADE_WAVES,       // k_shade register budget, waves per SIMD: 7 or 8 (-1: 7 for big non-instanced worlds)
  OPT_SHADE_BATCH,       // k_render: shade once this many lanes finished a segment
  OPT_TREELET_KB,        // LDS treelet per workgroup, KiB (0: none); applies at the next upload
  OPT_TRACE_BLOCK,       // k_trace workgroup size beside a treelet: 256, 512 or 1024
  OPT_MEM_RESERVE_MB,    // device memory a render leaves free when it sizes the pool and results slab
  OPT_TRAVERSAL,         // 0: the reference's left-first walk; 1: the verified near-first walk; -1: per scene (MRT_TRAVERSAL_*)
  OPT_TRACE_NF_BATCH,    // near-first walk: lanes whose walks are over wait for this many to check their hits together (-1: = refill)
  OPT_NF_KAPPA_LOG2,     // near-first walk: rays whose generic-triangle kappa exceeds 2^v take the reference walk (-8: every ray the bound covers)
  OPT_SHADE_BIN,         // k_shade: group each workgroup's survivors by material kind and direction signs (1), and split the pool by y sign (2); -1: per scene
  OPT_TRACE_PRIM_RUN,    // k_trace: primitive run while this many lanes are at a primitive (65: off; -1: 32 near-first / off)
  kNumOpts
};
struct OptDef {
  const char* name;
  int64_t def, lo, hi;
};
// Behind the larger defaults:
//  * pool_paths: large on purpose. Every k_trace launch ends with a tail of
//    long rays on few lanes, so the more rays a launch carries the smaller
//    that tail's share (measured on SphereGrid 1080p: 2M paths 186, 16M 377,
//    64M 434 Msamples/s; round 3, 256-spp steps: 64M 674, 128M 716, 256M 762,
//    384M 777, 544M 770). 384M paths hold 66 GiB of HBM (176 B each); a
//    render allocates min(samples per chunk, pool_paths).
//  * finish_paths: a queue whose work is exhausted hands its last paths to
//    one fused k_render launch (adopt mode) instead of per-bounce launches.
//    500k measured best (profiles/r2_experiments/finish_sweep.txt): mesh_ply
//    545 -> 678, sphere_grid 638 -> 642 Msamples/s.
//  * treelet_kb: off. Measured: the treelet removes the global
//    load of a step only when every lane of the wave is in the copy, and the
//    TA cost is per wave instruction, not per lane — 256/16 KB and 1024/78 KB
//    were 1% and 1-4% slower than no treelet.
constexpr OptDef kOptDefs[kNumOpts] = {
    {"queues", 2, 1, kMaxQueues},
    {"pool_paths", (int64_t)384 << 20, 1 << 16, 1 << 30},
    {"results_log2", 31, 10, 31},
    {"finish_paths", 500000, 0, 1 << 30},
    {"finish_grid_div", 1, 1, 64},
    {"trace_refill", -1, -1, 64},
    {"trace_box_min", -1, -1, 65},
    {"trace_chunk", -1, -1, 1 << 20},
    {"trace_prim_batch", 1, 1, 64},
    {"trace_wgs_per_cu", 0, 0, 32},
    {"shade_waves", -1, -1, 8},
    {"shade_batch", 16, 1, 64},
    {"treelet_kb", 0, 0, 150},
    {"trace_block", 256, 256, 1024},
    {"mem_reserve_mb", 4096, 0, 1 << 20},
    {"traversal", -1, -1, 1},
    {"trace_nf_batch", -1, -1, 64},
    {"nf_kappa_log2", -8, -40, -8},
    {"shade_bin", -1, -1, 2},
    {"trace_prim_run", -1, -1, 65},
};
inline int opt_find(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < kNumOpts; ++i)
    if (!strcmp(kOptDefs[i].name, name)) return i;
  return -1;
}

// Why value `v` cannot be stored in option `id`; empty: it can.
inline std::string opt_invalid(int id, int64_t v) {
  const OptDef& d = kOptDefs[id];
  if (v < d.lo || v > d.hi)
    return std::string("option ") + d.name + " out of range [" + std::to_string(d.lo) + ", " + std::to_string(d.hi) + "]";
  if (id == OPT_TRACE_BLOCK && v != 256 && v != 512 && v != 1024) return "option trace_block must be 256, 512 or 1024";
  if (id == OPT_SHADE_WAVES && v != -1 && v != 7 && v != 8) return "option shade_waves must be 7, 8 or -1 (per scene)";
  if (id == OPT_TRACE_NF_BATCH && v == 0) return "option trace_nf_batch must be 1..64 or -1";
  if (id == OPT_TRACE_PRIM_RUN && v == 0) return "option trace_prim_run must be 1..65 or -1";
  if (id == OPT_TRACE_CHUNK && v != -1 && v < 64) return "option trace_chunk must be >= 64 or -1";
  return "";
}

// Scheduling knobs of the persistent loops (kernel arguments so that they can
// be tuned without a rebuild: options "trace_refill", "trace_chunk", ...).
struct TraceTune {
  uint32_t chunk;        // rays per atomic grab
  uint32_t refill;       // refill once this many lanes idle
  uint32_t prim_batch;   // run the primitive branch once this many lanes wait at one
  uint32_t box_min;      // inner box loop while this many lanes are at a box (65: off)
  uint32_t shade_batch;  // k_render: shade once this many lanes finished a segment
  uint32_t nf_batch;     // near-first walk: check the hits once this many lanes' walks are over
  uint32_t prim_run;     // primitive steps alone while this many lanes are at a primitive (65: off)
};

// What the per-scene rules know about the uploaded scene (before one: nothing).
struct SceneFacts {
  bool big = false;        // the record stream is past half the chip's L2
  uint32_t instances = 0;  // instance count
  bool nf_trees = false;   // the scene has verified near-first trees (nf_tree.cpp)
  bool treelet = false;    // the scene has an LDS treelet
  bool trav_rng = false;   // the traversal draws random numbers (Volume, Mix alpha tests)
};

// Every value the loop derives from the options and the scene.
struct Tuning {
  TraceTune trace;
  bool use_nf;                             // k_trace walks the near-first trees
  int queues, trace_block;                 // path pools in use; k_trace workgroup size with a treelet
  int shade_wpe, shade_bin;                // k_shade: register budget (8 or 7 waves/SIMD); survivor grouping (0, 1, 2)
  int nf_kappa_log2;                       // near-first walk: kappa limit 2^v (DevScene::nfb.kmax)
  uint32_t finish_paths, finish_grid_div;  // drain hand-off: threshold (0: never); 1/div of its occupancy grid
  uint32_t wgs_per_cu, treelet_kb;         // persistent grids: workgroups per CU (0: occupancy); treelet KiB at the next upload
  size_t pool_paths, mem_reserve;          // live paths at most over all queues; bytes a render leaves free
  uint64_t results_max;                    // samples per results slab at most (16 B each)
};

// Options left at -1 take the per-scene rules:
//  * box run / refill (profiles/r2_tune, r3_tune.txt): refill 32
//    except 12 for a big instanced world (Menger 50.0 -> 53.0 at 64 spp per
//    step, 57.4 -> 58.8 at 256 with 16; mesh_ply keeps 32: 1148.7 vs 1125.9
//    at 24; profiles/r5_nf_probe/summary.txt); box run while >= 16 lanes are at a box for an
//    instance-heavy world (cube_field 266 -> 275, Menger 37.3 -> 44.1
//    Msamples/s), >= 32 for another stream past half the chip's L2 (its
//    record round trips go to the Infinity Cache; mesh_ply 749 -> 775), else
//    >= 24 (sphere_grid);
//  * rays per grab (profiles/r3_tune2/): an L2-resident world without many
//    instances runs longer stretches of neighbouring rays per wave
//    (sphere_grid 762.8 / 775.0 / 780.3 / 780.6 at 128 / 256 / 512 / 1024),
//    while big or instanced worlds keep 128 (mesh_ply 897.4 -> 841.4 at 1024:
//    its waves end on longer tails);
//  * k_shade at 7 waves/SIMD for a big non-instanced world (mesh_ply 948.6
//    -> 969.0), else 8 (sphere_grid 808.8, 7: 778.1; profiles/r3_tune2/wpe.txt).
//  The near-first walk (round 4, profiles/r4_nf/tune.txt) has rules of its
//  own: refill 40 except for a big non-instanced world (sphere_grid 1106.9
//  -> 1137.4, cube_field 608.6 -> 614.6; mesh_ply 1581.6 -> 1528.7 keeps 32)
//  (round 6: a big solid world grabs 256, mesh_ply 1274 -> 1290; profiles/r6_knobs/)
//  and box run >= 20 lanes without many instances (round 6, profiles/r6_knobs/:
//  mesh_ply 1213 -> 1252 from 28, sphere_grid 1155 -> 1164 from 24), 512 rays per grab except there (cube_field
//  556.2 -> 580.2 with shade 7; mesh_ply keeps 128: 1386.7 vs 1372.7), and
//  k_shade at 7 waves/SIMD everywhere (sphere_grid 983.3 -> 992.9).
inline Tuning derive_tuning(const int64_t* o, const SceneFacts& f) {
  Tuning t{};
  const bool inst = f.instances > 1000, big = f.big;
  t.treelet_kb = (uint32_t)o[OPT_TREELET_KB];
  // traversal -1 (per scene): the near-first walk unless the world is a big
  // instanced one (Menger 25.7 / 45.9 at trace_nf_batch 64 vs 50.0;
  // profiles/r5_walk_ab/). Round 5 also declined a margin with the generic-
  // triangle term (mesh_ply 548 vs 1148: |det| >= 1e-6 priced for every
  // ray); the normal cones and the wild instances' own tests turned that
  // around (mesh_ply 1228 vs 1152, profiles/r6_wild/)
  const bool nf_rule = !(inst && big);
  t.use_nf = (o[OPT_TRAVERSAL] == MRT_TRAVERSAL_NEAR_FIRST || (o[OPT_TRAVERSAL] < 0 && nf_rule)) && f.nf_trees &&
             !f.treelet && !f.trav_rng;
  const bool nf = t.use_nf, big_solid = big && !inst;
  t.queues = (int)o[OPT_QUEUES];
  t.pool_paths = (size_t)o[OPT_POOL_PATHS];
  t.results_max = 1ull << o[OPT_RESULTS_LOG2];
  t.finish_paths = (uint32_t)o[OPT_FINISH_PATHS];
  t.finish_grid_div = (uint32_t)o[OPT_FINISH_GRID_DIV];
  t.trace.refill = o[OPT_TRACE_REFILL] >= 0 ? (uint32_t)std::max<int64_t>(1, o[OPT_TRACE_REFILL])
                                            : ((nf && !big_solid) ? 40u : (inst && big) ? 12u : 32u);
  t.trace.box_min = o[OPT_TRACE_BOX_MIN] >= 0 ? (uint32_t)std::max<int64_t>(1, o[OPT_TRACE_BOX_MIN])
                                              : (inst ? 16u : (nf ? 20u : (big ? 32u : 24u)));
  t.trace.chunk = o[OPT_TRACE_CHUNK] >= 0 ? (uint32_t)o[OPT_TRACE_CHUNK]
                                          : (nf ? (big_solid ? 256u : 512u) : ((big || inst) ? 128u : 512u));
  t.trace.prim_batch = (uint32_t)o[OPT_TRACE_PRIM_BATCH];
  // primitive run (round 6, profiles/r6_primrun/): near-first walk 32
  // (mesh_ply 1365 -> 1392, sphere_grid 1206 -> 1229, cube_field 592 -> 605);
  // the reference walk's kernel has no primitive run (k_trace)
  t.trace.prim_run = o[OPT_TRACE_PRIM_RUN] > 0 ? (uint32_t)o[OPT_TRACE_PRIM_RUN] : (nf ? 32u : 65u);
  // A run that is on (<= 64) starts no sooner than the batch: k_trace's run
  // loop ends only when a pass finds the run over, so every pass must step a
  // lane. With prim_run >= prim_batch, "run" implies "go" for the lanes at a
  // primitive, and with the run off the lanes at a box step. (Below the
  // batch, a wave with prim_run <= lanes at a primitive < prim_batch and one
  // lane at a box stepped nobody, forever.) The thresholds only order the
  // lanes' steps: images and counters cannot change.
  if (t.trace.prim_run <= 64) t.trace.prim_run = std::max(t.trace.prim_run, t.trace.prim_batch);
  t.trace.nf_batch = o[OPT_TRACE_NF_BATCH] > 0 ? (uint32_t)o[OPT_TRACE_NF_BATCH] : t.trace.refill;
  t.trace.shade_batch = (uint32_t)o[OPT_SHADE_BATCH];
  t.shade_wpe = o[OPT_SHADE_WAVES] >= 0 ? (int)o[OPT_SHADE_WAVES] : ((nf || big_solid) ? 7 : 8);
  t.trace_block = (int)o[OPT_TRACE_BLOCK];
  t.mem_reserve = (size_t)o[OPT_MEM_RESERVE_MB] << 20;
  t.wgs_per_cu = (uint32_t)o[OPT_TRACE_WGS_PER_CU];
  t.nf_kappa_log2 = (int)o[OPT_NF_KAPPA_LOG2];
  // survivors grouped by material kind and direction signs (round 5,
  // profiles/r5_shade_bin/): sphere_grid 974 -> 1035, cube_field 504 -> 535
  // Msamples/s (k_trace lane utilisation 0.731 -> 0.774: a wave walks rays
  // that go the same way); mesh_ply, C5, Menger within noise. The pool-wide
  // y-sign split (2) on top, its two counts in one 64-bit atomic per
  // workgroup: sphere_grid 1035 -> 1086, cube_field 538 -> 558 (utilisation
  // 0.774 -> 0.798), mesh_ply 1150 -> 1152, C5 1137 -> 1132
  // (profiles/r5_surv64/; with two 32-bit atomics mesh_ply lost 1151 -> 1134,
  // profiles/r5_shade_block/) — 2 where the near-first walk runs, else 1
  t.shade_bin = o[OPT_SHADE_BIN] >= 0 ? (int)o[OPT_SHADE_BIN] : (nf ? 2 : 1);
  return t;
}

}  // namespace mrt
