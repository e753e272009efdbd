// The planner of the runtime-plan LDS FFT engine (lds_fft.hip) as pure
// functions: the radix sequence of a length, how many rows or columns one
// workgroup transforms, the split (four-step) factors of a column length and
// the tile geometry of a split pass. Nothing from HIP: conv.hip and
// lds_fft.hip call it, and tests/lds_fft_plan_query.cc prints it on the CPU
// (tests/test_lds_fft_plan.py asserts that every plan fits the register
// arrays StockhamPass declares and the LDS a workgroup may use).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rdl {

#ifndef RDL_FFT_THREADS
#define RDL_FFT_THREADS 1024
#endif
constexpr uint32_t kFftThreads = RDL_FFT_THREADS;

constexpr uint32_t kFftMaxPasses = 24;
constexpr size_t kFftLdsBytes = 160 * 1024;

// Complex elements one workgroup transforms at a time (count x length):
// bounds the butterflies per thread, hence registers (no spills at 512 threads).
constexpr uint32_t kMaxWgElems = 10240;

// Butterflies of radix R one thread of StockhamPass holds in registers
// (its v[BPT][R]): a workgroup's count x length / R butterflies must fit
// kFftThreads x BPT.
constexpr uint32_t StockhamBpt(uint32_t radix) {
  return (kMaxWgElems / radix + kFftThreads - 1) / kFftThreads;
}

// Double plans stop at radix 8 and 3: the composite radix-16 / radix-9
// butterflies hold twice their inputs in registers, which in double spills
// past the 128 VGPRs a 1024-thread workgroup leaves each wave (the spill
// traffic showed up as 4-5x the algorithmic HBM writes).
// Odd radices run first: the first pass writes its outputs R elements apart,
// and an odd stride spreads a wave's stores over the LDS banks where a
// power-of-two one piles them on a few (ds_write_b128: 8-way at stride 8).
inline bool Factorize(uint32_t n, bool f64, std::vector<uint8_t>& radix) {
  radix.clear();
  uint32_t m = n;
  uint32_t twos = 0;
  while (m % 2 == 0) {
    m /= 2;
    ++twos;
  }
  for (uint32_t r : {7u, 5u})
    while (m % r == 0) {
      m /= r;
      radix.push_back(uint8_t(r));
    }
  while (!f64 && m % 9 == 0) {
    m /= 9;
    radix.push_back(9);
  }
  while (m % 3 == 0) {
    m /= 3;
    radix.push_back(3);
  }
  const uint32_t big2 = f64 ? 3 : 4;
  while (twos >= big2) {
    radix.push_back(uint8_t(1u << big2));
    twos -= big2;
  }
  if (twos == 3) radix.push_back(8);
  if (twos == 2) radix.push_back(4);
  if (twos == 1) radix.push_back(2);
  return m == 1 && radix.size() <= kFftMaxPasses;
}

// The longest transform one workgroup can hold (either axis of a plane).
inline size_t LdsMaxLength(bool f64) {
  const size_t esz = f64 ? 16 : 8;
  return std::min<size_t>(kFftLdsBytes / esz, kMaxWgElems);
}

// Row pairs (length = width) or columns (length = height) per workgroup:
// fill ~64 KiB (float) / the LDS (double) so small planes still give each
// workgroup enough work; never more than LDS holds
inline uint32_t LdsTransformsPerWorkgroup(uint32_t length, bool f64) {
  const size_t esz = f64 ? 16 : 8;
  const size_t max_elems = LdsMaxLength(f64);
  const size_t budget = f64 ? kFftLdsBytes : 64 * 1024;
  uint32_t count = uint32_t(std::max<size_t>(1, std::min<size_t>(budget / (length * esz), 64)));
  count = std::min<uint32_t>(count, uint32_t(max_elems / length));
  return count;
}

// split columns: N = N1 * N2 with N1 the largest divisor <= sqrt(N); `cols`
// adjacent columns per tile: 256-byte row segments, as many as the
// sub-lengths allow
struct LdsSplitFactors {
  uint32_t n1, n2;
  bool can_split;
  uint32_t cols;
};

inline LdsSplitFactors ChooseLdsSplit(uint32_t height, bool f64) {
  LdsSplitFactors f{};
  uint32_t n1 = 1;
  for (uint32_t d = 1; uint64_t(d) * d <= height; ++d)
    if (height % d == 0) n1 = d;
  const uint32_t n2 = height / n1;
  f.n1 = n1;
  f.n2 = n2;
  f.can_split = n1 >= 4 && n2 >= 4;
  f.cols = std::max<uint32_t>(
      1, std::min<uint32_t>(f64 ? 16 : 32, kMaxWgElems / (std::max(n1, n2) + 1)));
  return f;
}

// One split pass (A over the n1 sub-length, B over n2) of a `width`-wide
// plane: `groups` sub-columns per tile out of n_groups, col_tiles tiles
// across the columns, the launch grid and its dynamic LDS bytes.
struct LdsSplitPass {
  uint32_t sub_len;
  uint32_t groups, n_groups;
  uint32_t n_cols, col_tiles;
  uint32_t grid;
  size_t lds;
};

inline LdsSplitPass PlanLdsSplitPass(uint32_t n1, uint32_t n2, uint32_t cols, bool f64,
                                     uint32_t width, bool pass_b) {
  LdsSplitPass p{};
  p.n_cols = width / 2 + 1;
  const uint32_t sub_len = pass_b ? n2 : n1;
  p.sub_len = sub_len;
  // elements per workgroup: half the LDS for double (two workgroups per CU
  // overlap one's loads with the other's transform), the engine's maximum
  // for float; the padded stride must fit as well
  const uint32_t target = f64 ? kMaxWgElems / 2 : kMaxWgElems;
  p.groups = std::max<uint32_t>(1, target / (cols * (sub_len + 1)));
  p.n_groups = pass_b ? n1 : n2;
  p.groups = std::min(p.groups, p.n_groups);
  p.col_tiles = (p.n_cols + cols - 1) / cols;
  p.grid = p.col_tiles * ((p.n_groups + p.groups - 1) / p.groups);
  p.lds = size_t(p.groups) * cols * (sub_len + 1) * (f64 ? 16 : 8);
  return p;
}

}  // namespace rdl
