// Prints the runtime LDS FFT planner's own answers (csrc/hip/lds_fft_plan.h),
// so that tests/test_lds_fft_plan.py and tests/test_lds_fft_sweep_gpu.py
// assert on the plans the library uses without restating them.
//
//   lds_fft_plan_query constants
//       C <threads> <max passes> <lds bytes> <max workgroup elements>
//       B <radix> <BPT>                       for radix 2..16
//   lds_fft_plan_query <n> <f64>
//   lds_fft_plan_query sweep <first> <last> <f64>
//       L <n> <f64> <factorized> <max length> <count> <radices or -> <can_split> <n1> <n2> <cols>
//     factorized: Factorize's return; a length is accepted when factorized and
//     n <= max length (rdl_conv_create_ex). count: rows pairs or columns per
//     workgroup (0 when n > max length). Radices comma-separated in pass order.
//   lds_fft_plan_query <w> <h> <f64> <columns>
//       P <w> <h> <f64> <ok> <row_count> <col_count> <split>
//       A|B <sub length> <groups> <n_groups> <n_cols> <col_tiles> <grid> <lds bytes>   (split only)
//     ok: 0 where rdl_conv_create_ex refuses the plane (a length not accepted,
//     or columns = 2 (RDL_CONV_COLUMNS_SPLIT) without a split).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lds_fft_plan.h"

namespace {

bool Accepted(uint32_t n, bool f64) {
  std::vector<uint8_t> radix;
  return n >= 2 && n <= rdl::LdsMaxLength(f64) && rdl::Factorize(n, f64, radix);
}

void PrintLength(uint32_t n, bool f64) {
  std::vector<uint8_t> radix;
  const bool ok = rdl::Factorize(n, f64, radix);
  const size_t max_len = rdl::LdsMaxLength(f64);
  const uint32_t count = n <= max_len ? rdl::LdsTransformsPerWorkgroup(n, f64) : 0;
  std::printf("L %u %d %d %zu %u ", n, int(f64), int(ok), max_len, count);
  if (!ok || radix.empty()) std::printf("-");
  for (size_t i = 0; ok && i < radix.size(); ++i)
    std::printf(i ? ",%u" : "%u", unsigned(radix[i]));
  const rdl::LdsSplitFactors s = rdl::ChooseLdsSplit(n, f64);
  std::printf(" %d %u %u %u\n", int(s.can_split), s.n1, s.n2, s.cols);
}

void PrintPass(const char* name, const rdl::LdsSplitPass& p) {
  std::printf("%s %u %u %u %u %u %u %zu\n", name, p.sub_len, p.groups, p.n_groups, p.n_cols,
              p.col_tiles, p.grid, p.lds);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "constants") == 0) {
    std::printf("C %u %u %zu %u\n", rdl::kFftThreads, rdl::kFftMaxPasses, rdl::kFftLdsBytes,
                rdl::kMaxWgElems);
    for (uint32_t r = 2; r <= 16; ++r) std::printf("B %u %u\n", r, rdl::StockhamBpt(r));
    return 0;
  }
  if (argc == 3) {
    PrintLength(uint32_t(std::atoll(argv[1])), std::atoi(argv[2]) != 0);
    return 0;
  }
  if (argc == 5 && std::strcmp(argv[1], "sweep") == 0) {
    const uint32_t first = uint32_t(std::atoll(argv[2])), last = uint32_t(std::atoll(argv[3]));
    for (uint32_t n = first; n <= last; ++n) PrintLength(n, std::atoi(argv[4]) != 0);
    return 0;
  }
  if (argc == 5) {
    const uint32_t w = uint32_t(std::atoll(argv[1])), h = uint32_t(std::atoll(argv[2]));
    const bool f64 = std::atoi(argv[3]) != 0;
    const int columns = std::atoi(argv[4]);
    const rdl::LdsSplitFactors s = rdl::ChooseLdsSplit(h, f64);
    const bool split = columns == 2;
    const bool ok = Accepted(w, f64) && Accepted(h, f64) && (!split || s.can_split);
    std::printf("P %u %u %d %d %u %u %d\n", w, h, int(f64), int(ok),
                ok ? rdl::LdsTransformsPerWorkgroup(w, f64) : 0,
                ok ? rdl::LdsTransformsPerWorkgroup(h, f64) : 0, int(ok && split));
    if (ok && split) {
      PrintPass("A", rdl::PlanLdsSplitPass(s.n1, s.n2, s.cols, f64, w, false));
      PrintPass("B", rdl::PlanLdsSplitPass(s.n1, s.n2, s.cols, f64, w, true));
    }
    return 0;
  }
  std::fprintf(stderr, "lds_fft_plan_query: see the comment at the top of the source\n");
  return 2;
}
