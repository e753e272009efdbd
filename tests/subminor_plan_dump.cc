// Prints PlanSubminorLoop over a fixed sweep of its domain, one row of
// integers per case: the inputs, then the plan. Distinct error texts follow
// as "E <id> <text>" lines (ids in order of first appearance, from 1).
// tests/test_subminor_plan.py compares the output with
// tests/golden/subminor_plan_parent.npz.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "rdl_hip.h"
#include "subminor_plan.h"

namespace {

struct Flags {
  bool copy, rms, spectral, logpoly;
  uint32_t integ_mode;
};
struct Env {
  uint32_t coop_limit;
  int n_cus;
  int tab;
  uint32_t tab_threads, big_target;
};

std::vector<std::string> error_texts;

int ErrorId(const char* text) {
  if (!text) return 0;
  for (size_t i = 0; i < error_texts.size(); ++i)
    if (error_texts[i] == text) return int(i) + 1;
  error_texts.push_back(text);
  return int(error_texts.size());
}

void Row(int mode, uint32_t target, uint64_t n_sel, uint32_t n_images, uint32_t n_pol,
         const Flags& f, const Env& e) {
  rdl::SubminorTuning t;  // the defaults, then rdl_subminor_set_tuning(mode, target)
  t.mode = mode;
  if (target) (mode == 6 ? t.tab_target : t.target_per_block) = target;
  t.tab = e.tab;
  t.tab_threads = e.tab_threads;
  t.big_target = e.big_target;
  rdl::SubminorShape s;
  s.n_sel = n_sel;
  s.n_images = n_images;
  s.n_pol = n_pol;
  s.integ_mode = f.integ_mode;
  s.copy_fast_path = f.copy;
  s.has_rms = f.rms;
  s.has_spectral = f.spectral;
  s.has_logpoly = f.logpoly;
  s.n_cus = e.n_cus;
  s.coop_limit = e.coop_limit;
  const rdl::LoopPlan p = rdl::PlanSubminorLoop(t, s);
  std::printf("%d %u %llu %u %u %u %d %d %d %d %d %u %d %u %u  %d %d %d %u %u %u %llu %d %llu %d %u %llu %u %d\n",
              mode, target, (unsigned long long)n_sel, n_images, n_pol, f.integ_mode,
              int(f.copy), int(f.rms), int(f.spectral), int(f.logpoly), e.n_cus, e.coop_limit,
              e.tab, e.tab_threads, e.big_target,
              ErrorId(p.error_text), p.error, int(p.kind), p.threads, p.items, p.n_blocks,
              (unsigned long long)p.per_block, int(p.use_lds), (unsigned long long)p.lds_bytes,
              int(p.build_table), p.part_stride, (unsigned long long)p.rec_bytes,
              p.ni_template, p.trace_kind);
}

}  // namespace

int main() {
  const rdl::SubminorTuning d;  // the thresholds come from the defaults
  // every threshold of the choice +-1, and values between
  std::set<uint64_t> n_full = {1, 40, 100, 200, 384, 700, 1500, 3000, 3800, 6000, 12000,
                               20000, 100000, 500000, 5000000};
  for (uint64_t b : {uint64_t(2), uint64_t(64), uint64_t(128), uint64_t(256), uint64_t(512),
                     uint64_t(1024), uint64_t(2048), uint64_t(4096), uint64_t(8192),
                     uint64_t(d.wave_max), uint64_t(d.single_max), uint64_t(d.big_max),
                     uint64_t(d.tab_single), uint64_t(d.table_max), uint64_t(256) * 4096,
                     uint64_t(1) << 24})
    for (uint64_t v : {b - 1, b, b + 1}) n_full.insert(v);
  // single_max, big_max and 8192 gathers per iteration with 3 and 5 images,
  // big_max with 2, 4 and 8; the table's size bound with 3, 4 and 5 PSFs
  for (uint64_t v : {682, 683, 409, 410, 1194, 1195, 716, 717, 448, 449, 896, 897, 1792, 1793,
                     2730, 2731, 1638, 1639, 11585, 11586, 13377, 13378, 10362, 10363})
    n_full.insert(v);
  const std::vector<uint64_t> n_short = {1,    100,  129,   1025,  2049,   3585,    4097,
                                         8192, 8193, 16384, 16385, 100000, 1048577, uint64_t(1) << 24};
  const std::vector<uint64_t> n_tab = {2,    129,  1024, 2048, 2049,  4096,  4097,
                                       8192, 8193, 9000, 12000, 16383, 16384, 16385};
  const uint32_t images[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 64};
  const uint32_t targets[] = {0, 512, 4096};
  // the table kernels' shapes (copy / joined linear), each with one condition
  // broken, and everything on
  const Flags q1{true, false, false, false, RDL_INTEGRATE_LINEAR};
  const Flags q2{false, false, false, false, RDL_INTEGRATE_LINEAR};
  const Flags flags[] = {q1,
                         q2,
                         {true, true, false, false, RDL_INTEGRATE_LINEAR},
                         {true, false, true, false, RDL_INTEGRATE_LINEAR},
                         {true, false, false, true, RDL_INTEGRATE_LINEAR},
                         {true, false, false, false, RDL_INTEGRATE_SQUARE},
                         {false, true, false, false, RDL_INTEGRATE_LINEAR},
                         {false, false, true, false, RDL_INTEGRATE_LINEAR},
                         {false, false, false, true, RDL_INTEGRATE_LINEAR},
                         {false, false, false, false, RDL_INTEGRATE_SQUARE},
                         {true, true, true, true, RDL_INTEGRATE_SQUARE}};
  const Env base{0, 256, 1, 0, 0};

  // 1: the sizes, images, modes and flags, on a whole GPU with the defaults
  for (uint64_t n_sel : n_full)
    for (uint32_t ni : images)
      for (uint32_t np : {1u, 2u})
        if (ni % np == 0)
          for (int mode = 0; mode <= 6; ++mode)
            for (uint32_t target : targets)
              for (const Flags& f : flags) Row(mode, target, n_sel, ni, np, f, base);
  // 2: pooled sessions, small GPUs, the table loop off, 1024-thread grids
  for (uint64_t n_sel : n_short)
    for (uint32_t ni : images)
      for (uint32_t np : {1u, 2u})
        if (ni % np == 0)
          for (int mode = 0; mode <= 6; ++mode)
            for (uint32_t target : targets)
              for (const Flags& f : {q1, q2})
                for (uint32_t coop : {0u, 16u})
                  for (int cus : {256, 32})
                    for (int tab : {1, 0})
                      for (uint32_t bt : {0u, 2048u}) {
                        const Env e{coop, cus, tab, 0, bt};
                        if (std::memcmp(&e, &base, sizeof(e)) != 0)
                          Row(mode, target, n_sel, ni, np, f, e);
                      }
  // 3: the table loop's workgroup size
  for (uint64_t n_sel : n_tab)
    for (uint32_t ni : {1u, 2u})
      for (int mode = 0; mode <= 6; ++mode)
        for (uint32_t target : targets)
          for (const Flags& f : {q1, q2})
            for (uint32_t coop : {0u, 16u})
              for (int cus : {256, 32})
                for (uint32_t tt : {256u, 1024u})
                  Row(mode, target, n_sel, ni, 1, f, Env{coop, cus, 1, tt, 0});
  for (size_t i = 0; i < error_texts.size(); ++i)
    std::printf("E %zu %s\n", i + 1, error_texts[i].c_str());
  return 0;
}
