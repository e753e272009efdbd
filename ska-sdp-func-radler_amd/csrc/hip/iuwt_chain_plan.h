// The row-chain kernels' launch geometry (IuwtDecomposeChain /
// IuwtRecomposeChain, iuwt.hip): the arguments of one launch and PlanChain,
// which lays a scale out as chains, segments and column strips or refuses it.
// A pure host function of five values, so the choice can be read in one
// piece and tested without a GPU (tests/test_iuwt_chain_plan.py checks, over
// a sweep of its domain, what the kernels need from a plan). Plain C++17;
// nothing from HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "div_up.h"

namespace rdl {

struct ChainArgs {
  const float* a;     // this scale's approximation (decompose) / the coarser
                      // recomposition (recompose)
  float* i1;          // next approximation (decompose) / finer recomposition
  float* coef;        // this scale's coefficients: written (decompose) or
                      // added (recompose)
  uint32_t w, h;
  int d;
  uint32_t ws;        // output columns per workgroup (multiple of 4, <= 1024)
  uint32_t n_strips;  // ceil(w / ws)
  uint32_t n_seg;     // segments per chain
  uint32_t n_res;     // chains: min(d, h) residues
  float* dummy;       // 256 floats: the stores of lanes with nothing to store
};

// the chain launch's geometry for spacing d, or false when the rows do not
// fit its register/LDS budget (the row kernels then run)
struct ChainPlan {
  ChainArgs a;
  unsigned blocks;
  size_t lds;
  int na, no, ni;  // float4 loads per thread per row; output and halo-strip
                   // columns per thread (multiples of 256)
};
inline bool PlanChain(uint32_t w, uint32_t h, int d, bool decompose, const char* ws_override,
                      ChainPlan* pl) {
  // 512 columns per workgroup at every spacing: 1024 (fewer halo columns at
  // d >= 31) lowers the occupancy more than it saves (r06 measurement)
  uint32_t ws = 512u;
  if (const char* e = ws_override) {  // RDL_IUWT_CHAIN_WS (measurement)
    const unsigned v = unsigned(std::atoi(e));
    if (v >= 256 && v <= 1024 && v % 256 == 0) ws = v;
  }
  if (ws > (w + 3u) / 4u * 4u) ws = (w + 3u) / 4u * 4u;
  const int64_t halo = decompose ? 4 * int64_t(d) : 2 * int64_t(d);
  const int64_t wa4 = (int64_t(ws) + 2 * halo + 6) / 4;
  if (wa4 > 512) return false;
  pl->na = wa4 <= 256 ? 1 : 2;
  pl->no = int(DivUp(ws, 256));
  if (pl->no == 3) pl->no = 4;
  const int64_t wi = int64_t(ws) + 4 * int64_t(d);
  pl->ni = std::max(pl->no, int((wi + 255) / 256));
  if (pl->ni > pl->no + 2) return false;
  const uint32_t n_strips = (w + ws - 1) / ws;
  const uint32_t n_res = uint32_t(d) < h ? uint32_t(d) : h;  // chains with rows
  const uint32_t k_max = (h + uint32_t(d) - 1) / uint32_t(d);
  uint32_t n_seg = std::min(DivUp(k_max, 24), DivUp(1536, size_t(n_res) * n_strips));
  n_seg = std::max(1u, std::min(n_seg, k_max));
  const uint64_t n_blocks = uint64_t(n_res) * n_seg * n_strips;
  if (n_blocks > (uint64_t(1) << 30)) return false;
  ChainArgs& a = pl->a;
  a.w = w;
  a.h = h;
  a.d = d;
  a.ws = ws;
  a.n_strips = n_strips;
  a.n_seg = n_seg;
  a.n_res = n_res;
  pl->blocks = unsigned(8 * ((n_blocks + 7) / 8));
  const int64_t slots = 2 * 1024 * int64_t(pl->na);
  pl->lds = decompose ? size_t(slots + 7 * wi + 11 * int64_t(ws)) * sizeof(float)
                      : size_t(slots + 5 * int64_t(ws)) * sizeof(float);
  return pl->lds <= 160 * 1024;
}

}  // namespace rdl
