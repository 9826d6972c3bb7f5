// options_check — the context options and their per-scene rules on the host
// (csrc/host/options.h), for tests/test_options.py.
//   options_check [fact=value ...] [option=value ...]
//     facts: big, instances, nf_trees, treelet, trav_rng. Options are
//     validated like mrt_set_option; prints the derived Tuning, one
//     "name value" per line, or "error: <text>" (exit 1).
//   options_check prim_sweep [fact=value ...] [option=value ...]
//     the same for every trace_prim_batch in 1..64 and trace_prim_run in
//     {-1, 1..65}: one line "batch run prim_batch prim_run" each.
#include <stdio.h>
#include <stdlib.h>

#include "../mass-raytrace_amd/csrc/host/options.h"

using namespace mrt;

static void print_tuning(const Tuning& t) {
  printf("queues %d\npool_paths %zu\nresults_max %llu\nfinish_paths %u\nfinish_grid_div %u\n", t.queues, t.pool_paths,
         (unsigned long long)t.results_max, t.finish_paths, t.finish_grid_div);
  printf("trace_refill %u\ntrace_box_min %u\ntrace_chunk %u\ntrace_prim_batch %u\ntrace_prim_run %u\n", t.trace.refill,
         t.trace.box_min, t.trace.chunk, t.trace.prim_batch, t.trace.prim_run);
  printf("trace_nf_batch %u\nshade_batch %u\nwgs_per_cu %u\nmem_reserve %zu\ntreelet_kb %u\ntrace_block %d\n",
         t.trace.nf_batch, t.trace.shade_batch, t.wgs_per_cu, t.mem_reserve, t.treelet_kb, t.trace_block);
  printf("traversal %d\nshade_waves %d\nshade_bin %d\nnf_kappa_log2 %d\n", t.use_nf ? 1 : 0, t.shade_wpe, t.shade_bin,
         t.nf_kappa_log2);
}

int main(int argc, char** argv) {
  int64_t opt[kNumOpts];
  for (int i = 0; i < kNumOpts; ++i) opt[i] = kOptDefs[i].def;
  SceneFacts f;
  bool sweep = false;
  for (int a = 1; a < argc; ++a) {
    std::string arg = argv[a];
    if (arg == "prim_sweep") {
      sweep = true;
      continue;
    }
    const size_t eq = arg.find('=');
    if (eq == std::string::npos) return printf("error: expected name=value, got %s\n", argv[a]), 2;
    const std::string name = arg.substr(0, eq);
    const int64_t v = strtoll(arg.c_str() + eq + 1, nullptr, 10);
    if (name == "big") f.big = v != 0;
    else if (name == "instances") f.instances = (uint32_t)v;
    else if (name == "nf_trees") f.nf_trees = v != 0;
    else if (name == "treelet") f.treelet = v != 0;
    else if (name == "trav_rng") f.trav_rng = v != 0;
    else {
      const int id = opt_find(name.c_str());
      if (id < 0) return printf("error: unknown option %s\n", name.c_str()), 1;
      const std::string why = opt_invalid(id, v);
      if (!why.empty()) return printf("error: %s\n", why.c_str()), 1;
      opt[id] = v;
    }
  }
  if (!sweep) {
    print_tuning(derive_tuning(opt, f));
    return 0;
  }
  for (int64_t batch = 1; batch <= 64; ++batch)
    for (int64_t run = -1; run <= 65; ++run) {
      if (run == 0) continue;
      if (!opt_invalid(OPT_TRACE_PRIM_BATCH, batch).empty() || !opt_invalid(OPT_TRACE_PRIM_RUN, run).empty())
        return printf("error: %lld / %lld rejected\n", (long long)batch, (long long)run), 1;
      opt[OPT_TRACE_PRIM_BATCH] = batch;
      opt[OPT_TRACE_PRIM_RUN] = run;
      const Tuning t = derive_tuning(opt, f);
      printf("%lld %lld %u %u\n", (long long)batch, (long long)run, t.trace.prim_batch, t.trace.prim_run);
    }
  return 0;
}
