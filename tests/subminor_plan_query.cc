// Prints PlanSubminorLoop's answer for one launch, so a GPU test can assert
// which loop kernel its run used without restating the plan's thresholds
// (tests/test_subminor_options_gpu.py). Arguments, all integers:
//   mode target n_sel n_images n_pol integ_mode copy_fast_path has_rms
//   has_spectral has_logpoly n_cus coop_limit table_max
// mode and target as given to rdl_subminor_set_tuning (target 0 = keep);
// table_max < 0 keeps the default (RDL_SUBMINOR_TABLE_MAX otherwise). Every
// other tuning value is the default. Output, one line:
//   error kind n_blocks build_table use_lds threads items
#include <cstdio>
#include <cstdlib>

#include "rdl_hip.h"
#include "subminor_plan.h"

int main(int argc, char** argv) {
  if (argc != 14) {
    std::fprintf(stderr, "subminor_plan_query: 13 arguments expected\n");
    return 2;
  }
  long long v[13];
  for (int i = 0; i < 13; ++i) v[i] = std::atoll(argv[i + 1]);
  rdl::SubminorTuning t;
  t.mode = int(v[0]);
  if (v[1]) (t.mode == 6 ? t.tab_target : t.target_per_block) = uint32_t(v[1]);
  if (v[12] >= 0) t.table_max = uint32_t(v[12]);
  rdl::SubminorShape s;
  s.n_sel = uint64_t(v[2]);
  s.n_images = uint32_t(v[3]);
  s.n_pol = uint32_t(v[4]);
  s.integ_mode = uint32_t(v[5]);
  s.copy_fast_path = v[6] != 0;
  s.has_rms = v[7] != 0;
  s.has_spectral = v[8] != 0;
  s.has_logpoly = v[9] != 0;
  s.n_cus = int(v[10]);
  s.coop_limit = uint32_t(v[11]);
  const rdl::LoopPlan p = rdl::PlanSubminorLoop(t, s);
  std::printf("%d %d %u %d %d %u %u\n", p.error, int(p.kind), p.n_blocks, int(p.build_table),
              int(p.use_lds), p.threads, p.items);
  return 0;
}
