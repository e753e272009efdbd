// What the sub-minor loop's translation units share: the handle, the loop
// kernels' arguments and result, the argmax key, the write-through and
// cross-lane helpers, and the host functions each unit offers the others
// (subminor.hip holds the sequence that calls them). The device functions
// that only the loop kernels share are in subminor_loop_shared.h.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "rdl_internal.h"
#include "logpoly.h"
#include "subminor_plan.h"

struct rdl_subminor {
  rdl_session* s = nullptr;
  void* counts = nullptr;  // per-chunk counts / offsets
  size_t counts_bytes = 0;
  void* sel = nullptr;     // positions + R + M for the selected set
  size_t sel_bytes = 0;
  void* sync = nullptr;    // records + counter + result + trace
  size_t sync_bytes = 0;
  uint64_t n_selected = 0;
  uint32_t n_images = 0;
  uint32_t width = 0, height = 0;
  uint32_t* d_pos = nullptr;
  float* d_r = nullptr;
  float* d_m = nullptr;
  rdl::SubminorTuning tuning;         // the loop kernel choice (PlanSubminorLoop)
  void* table = nullptr;             // [n_psf][n_sel][n_sel] PSF values at the
  size_t table_bytes = 0;             //   selected pixels' pairwise offsets
  void* pos_buf = nullptr;            // selected positions (sparse / single pass)
  size_t pos_bytes = 0;
  void* local_buf = nullptr;          // sparse selection: the chunks' own lists
  size_t local_bytes = 0;
  void* stamp_mark = nullptr;         // shape-model stamping: tiles a stamp reaches
  size_t stamp_mark_bytes = 0;
  int select_passes = 0;              // 0 sparse two-phase, 1 single pass, 3 count + scan + scatter
  int select_ticket = 1;              // single pass: chunk order by ticket
  int select_quad = 1;                // sparse: 16-byte loads where they apply
  uint64_t select_spin_limit = uint64_t(1) << 26;  // look-back polls before failing
  // a launched loop whose result has not been read (rdl_subminor_launch ->
  // rdl_subminor_collect)
  bool pending = false;
  uint64_t pending_start = 0;       // iteration_start of the launch
  double pending_bytes_per_it = 0;  // algorithmic bytes per iteration
  const uint32_t* pending_result = nullptr;
  hipEvent_t pending_ev0 = nullptr, pending_ev1 = nullptr;  // RDL_TRACE_SUBMINOR
  uint64_t pending_n_sel = 0;
  uint32_t pending_g = 0;
  int pending_kind = 0, pending_threads = 0, pending_table = 0;
};

namespace rdl {

// ----------------------------------------------------------------- loop
struct LoopArgs {
  const uint32_t* pos;    // n_sel
  float* r;               // [n_img][n_sel] (in: gathered residuals)
  float* m;               // [n_img][n_sel] (out: model values)
  const float* psfs;      // twice-convolved PSFs, W*H planes
  const float* spectral;  // n_img x n_img spectral-fit map, or nullptr
  const float* rms;       // RMS factor image (W x H), or nullptr
  uint32_t* records;      // [2][G][rec_words] (G > 1)
  uint32_t* counter;      // arrival counter (G > 1), zeroed per launch
  uint32_t* result;       // LoopResult
  uint32_t* trace;        // 2 x u32 per component
  uint64_t trace_cap;
  uint64_t n_sel;
  uint32_t per_block;
  uint32_t n_blocks;
  uint32_t rec_words;
  uint32_t width, height, n_img, n_pol;
  rdl_integration integ;
  float threshold, gain, divergence_limit;
  uint64_t iteration_start, max_iterations;
  int32_t allow_negative, stop_on_negative;
  int32_t use_lds;
  int32_t prof;           // accumulate per-phase cycles (block 0, wave 0)
  const float* table;     // pairwise PSF table (BuildPairTable) or nullptr
  rdl_logpoly lp;         // log-polynomial fit (has_lp; SubminorLoop only)
  int32_t has_lp;
  int32_t has_forced;     // forced-term fit with lp's channels (needs has_lp)
  rdl_forced_terms forced;
  // table loops on a grid: launched blocks per participant (the participants
  // are blocks 0, S, 2S, ...: S = 8 puts them on one XCD under round-robin
  // dispatch; a pooled session whose share of the GPU is below 8 blocks per
  // participant launches S = 1), and 1 to exchange through agent-scope
  // stores even when every participant is on one XCD (RDL_SUBMINOR_EXCHANGE=agent)
  uint32_t part_stride;
  int32_t agent_exchange;
  // SubminorLoopTab with one workgroup: the block argmax as ONE 64-bit LDS
  // atomic max per 16-lane row (RDL_SUBMINOR_ATOMIC=0: the wave slots)
  int32_t atomic_reduce;
};

struct LoopResult {
  uint64_t iteration;
  float peak;
  int32_t diverging;
  float flux;
  uint32_t error;
};

__device__ __forceinline__ uint64_t MaxKey(float integ, bool allow_negative,
                                           uint64_t p) {
  const float v = allow_negative ? fabsf(integ) : integ;
  if (v != v) return 0ull;  // NaN never wins (unless everything is NaN)
  uint32_t u = __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (uint64_t(u) << 32) | uint64_t(0xffffffffu - uint32_t(p));
}

// The float MaxKey encoded (|v| when allow_negative).
__device__ __forceinline__ float KeyValue(uint64_t key) {
  uint32_t u = uint32_t(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}

__device__ __forceinline__ void StoreSc1(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t LoadSc1(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the pairwise PSF table's mark for an offset outside the PSF plane
constexpr uint32_t kOutsideBits = 0x7fbadbadu;  // a NaN payload no PSF value carries

// DPP cross-lane moves (gfx9 family): a 64-lane max in 6 VALU steps instead
// of 6 ds_bpermute round trips; the result is read from lane 63 (or lane 0
// for the 8-lane form) into a scalar.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ uint64_t DppU64(uint64_t v) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_update_dpp(
      0, int(uint32_t(v)), CTRL, ROW_MASK, 0xf, false));
  const uint32_t hi = uint32_t(__builtin_amdgcn_update_dpp(
      0, int(uint32_t(v >> 32)), CTRL, ROW_MASK, 0xf, false));
  return (uint64_t(hi) << 32) | lo;
}
__device__ __forceinline__ uint64_t ReadLaneU64(uint64_t v, int lane) {
  const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), lane));
  const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), lane));
  return (uint64_t(hi) << 32) | lo;
}
// Max over lanes 0..7 (others must hold 0); uniform result.
__device__ __forceinline__ uint64_t Max8U64(uint64_t v) {
  uint64_t t;
  t = DppU64<0xb1>(v);  // quad_perm [1,0,3,2]
  v = t > v ? t : v;
  t = DppU64<0x4e>(v);  // quad_perm [2,3,0,1]
  v = t > v ? t : v;
  t = DppU64<0x141>(v);  // row_half_mirror
  v = t > v ? t : v;
  return ReadLaneU64(v, 0);
}
// Max over lanes 0..15 (others must hold 0); uniform result.
__device__ __forceinline__ uint64_t Max16U64(uint64_t v) {
  uint64_t t;
  t = DppU64<0xb1>(v);
  v = t > v ? t : v;
  t = DppU64<0x4e>(v);
  v = t > v ? t : v;
  t = DppU64<0x141>(v);
  v = t > v ? t : v;
  t = DppU64<0x140>(v);  // row_mirror
  v = t > v ? t : v;
  return ReadLaneU64(v, 0);
}
// Max over the 64 lanes; uniform result.
__device__ __forceinline__ uint64_t Max64U64(uint64_t v) {
  uint64_t t;
  t = DppU64<0xb1>(v);
  v = t > v ? t : v;
  t = DppU64<0x4e>(v);
  v = t > v ? t : v;
  t = DppU64<0x141>(v);
  v = t > v ? t : v;
  t = DppU64<0x140>(v);  // row_mirror
  v = t > v ? t : v;
  t = DppU64<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
  v = t > v ? t : v;
  t = DppU64<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
  v = t > v ? t : v;
  return ReadLaneU64(v, 63);
}
// Workgroup barrier that orders LDS only: __syncthreads() also drains vmcnt,
// which would make every iteration wait for its own trace/granule stores.
__device__ __forceinline__ void LdsBarrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ int FirstLane(bool pred) {
  const uint64_t b = __ballot(pred);
  return b ? __builtin_ctzll(b) : 0;
}

// 32-bit max over lanes (DPP, one fused max per step); LANES = 8, 16 or 64
// (lanes beyond LANES must hold 0); uniform result.
template <int LANES>
__device__ __forceinline__ uint32_t MaxU32(uint32_t v) {
  auto step = [](uint32_t x, uint32_t t) { return x > t ? x : t; };
  v = step(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xb1, 0xf, 0xf, false)));
  v = step(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x4e, 0xf, 0xf, false)));
  v = step(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x141, 0xf, 0xf, false)));
  if constexpr (LANES == 8) return uint32_t(__builtin_amdgcn_readlane(int(v), 0));
  v = step(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x140, 0xf, 0xf, false)));
  if constexpr (LANES == 16) return uint32_t(__builtin_amdgcn_readlane(int(v), 0));
  v = step(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xa, 0xf, false)));
  v = step(v, uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xc, 0xf, false)));
  return uint32_t(__builtin_amdgcn_readlane(int(v), 63));
}

// The largest 64-bit argmax key over lanes and its lane (the lowest lane
// holding it; lane 0 when every key is 0). The value word (high half) is
// reduced alone; the index word only settles exact value ties, which are
// rare (keys are unique per pixel, and a high word of 0 means a 0 key).
template <int LANES>
__device__ __forceinline__ uint64_t KeyMax(uint64_t key, int& lane_out) {
  const uint32_t hi = uint32_t(key >> 32);
  const uint32_t mh = MaxU32<LANES>(hi);
  if (mh == 0u) {
    lane_out = 0;
    return 0ull;
  }
  const uint64_t tie = __ballot(hi == mh);
  if ((tie & (tie - 1ull)) == 0ull) {
    lane_out = __builtin_ctzll(tie);
    return (uint64_t(mh) << 32) |
           uint32_t(__builtin_amdgcn_readlane(int(uint32_t(key)), lane_out));
  }
  const uint64_t k = hi == mh ? key : 0ull;
  const uint64_t m = LANES == 8 ? Max8U64(k) : LANES == 16 ? Max16U64(k) : Max64U64(k);
  lane_out = FirstLane(key == m);
  return m;
}

// One loop launch: a cooperative grid when workgroups exchange their winners,
// else one workgroup.
template <typename Kernel>
int LaunchLoopKernel(Kernel kernel, uint32_t grid, uint32_t threads, size_t lds_bytes,
                     const LoopArgs& a, hipStream_t stream) {
  if (a.n_blocks > 1) {
    void* args[] = {const_cast<LoopArgs*>(&a)};
    RDL_HIP_CHECK(hipLaunchCooperativeKernel(reinterpret_cast<const void*>(kernel), dim3(grid),
                                             dim3(threads), args, unsigned(lds_bytes), stream));
  } else {
    kernel<<<1, threads, lds_bytes, stream>>>(a);
    RDL_HIP_CHECK(hipGetLastError());
  }
  return RDL_OK;
}

// (re)allocates *p when it holds fewer than `need` bytes (subminor.hip)
int Grow(void** p, size_t* have, size_t need, hipStream_t stream);
// subminor_select.hip: the selected pixels' positions and residual values
// into h->d_pos / h->d_r (h->d_m: their model values), their count to *n_sel
int RunSelection(rdl_subminor* h, const float* d_residuals, const rdl_subminor_params* p,
                 uint64_t* n_sel);
// the launch of the plan's kernel: subminor_loop_lds.hip (LoopKind::Lds),
// subminor_loop_reg.hip (Reg, Wave, Big), subminor_loop_tab.hip (Tab, TabN)
int LaunchLdsLoop(const LoopArgs& a, const LoopPlan& plan, hipStream_t stream);
int LaunchRegLoop(const LoopArgs& a, const LoopPlan& plan, hipStream_t stream);
int LaunchTabLoop(const LoopArgs& a, const LoopPlan& plan, hipStream_t stream);
// subminor_loop_tab.hip: the n_psf x n_sel x n_sel table; also zeroes
// zero_words 8-byte words at `zero` (the loop's exchange area)
int LaunchPairTable(const uint32_t* pos, const float* psfs, uint32_t n_sel, uint32_t n_psf,
                    uint32_t width, uint32_t height, float* table, uint64_t* zero,
                    uint32_t zero_words, hipStream_t stream);

}  // namespace rdl
