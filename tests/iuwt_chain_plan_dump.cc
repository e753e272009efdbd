// Prints PlanChain (csrc/hip/iuwt_chain_plan.h) over a fixed sweep of its
// domain, one row of integers per case:
//   w h d decompose ws_override  ok ws n_strips n_seg n_res blocks lds na no ni
// (ws_override 0: none; a refused plan prints zeros after ok = 0).
// tests/test_iuwt_chain_plan.py checks what the kernels need from every row.
//
// The kernel instantiation depends on (min(ws, w rounded up to 4), d) alone,
// so every width that is a multiple of 4 up to 1028 with every spacing
// reaches all of them; the heights and the larger widths vary the chains,
// segments and workgroup counts.
#include <cstdio>
#include <set>
#include <vector>

#include "iuwt_chain_plan.h"

namespace {

void Row(uint32_t w, uint32_t h, int d, bool decompose, int ws_override) {
  char text[16];
  std::snprintf(text, sizeof text, "%d", ws_override);
  rdl::ChainPlan p{};
  const bool ok = rdl::PlanChain(w, h, d, decompose, ws_override ? text : nullptr, &p);
  if (!ok) p = rdl::ChainPlan{};
  std::printf("%u %u %d %d %d %d %u %u %u %u %u %zu %d %d %d\n", w, h, d, int(decompose),
              ws_override, int(ok), p.a.ws, p.a.n_strips, p.a.n_seg, p.a.n_res, p.blocks, p.lds,
              p.na, p.no, p.ni);
}

void Sweep(const std::vector<uint32_t>& ws, const std::vector<uint32_t>& hs) {
  for (uint32_t w : ws)
    for (uint32_t h : hs)
      for (int k = 1; k <= 12; ++k)
        for (bool decompose : {true, false})
          for (int ov : {0, 256, 768, 1024}) Row(w, h, (1 << k) - 1, decompose, ov);
}

}  // namespace

int main() {
  std::vector<uint32_t> w_all;
  for (uint32_t w = 4; w <= 1028; w += 4) w_all.push_back(w);
  for (uint32_t w : {1280u, 1532u, 1536u, 1540u, 2048u, 2052u, 3072u, 4096u, 8192u, 16380u,
                     16384u, 16388u})
    w_all.push_back(w);
  const std::vector<uint32_t> h_few = {1, 37, 300};
  const std::vector<uint32_t> w_few = {4,    8,    64,   256,  260,  300,  512,   516,  520,
                                       1000, 1024, 1028, 2048, 4096, 8192, 16384, 16388};
  std::set<uint32_t> h_set;
  for (uint32_t h = 1; h <= 32; ++h) h_set.insert(h);
  for (int k = 1; k <= 10; ++k)  // d and 2d, +-1
    for (uint32_t m : {1u, 2u})
      for (int e : {-1, 0, 1}) {
        const int64_t h = int64_t(m) * ((1 << k) - 1) + e;
        if (h >= 1 && h <= 1100) h_set.insert(uint32_t(h));
      }
  for (uint32_t h : {37u, 40u, 48u, 100u, 131u, 200u, 260u, 300u, 600u, 1000u, 1100u})
    h_set.insert(h);
  Sweep(w_all, h_few);
  Sweep(w_few, std::vector<uint32_t>(h_set.begin(), h_set.end()));
  return 0;
}
