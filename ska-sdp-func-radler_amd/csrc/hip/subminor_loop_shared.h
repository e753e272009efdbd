// The rules of the sub-minor loop that its kernels share, each written once
// (device code only; every function is inlined into its kernel):
//   all four kernels   WriteTrace, WriteResult
//   Tab and TabN       ThreadBestAbs, LexMaxLane, XccHandshake
// All but ThreadBestAbs, which reads the thread's value array through a
// reference, take values and return values. A helper that is handed the
// kernel's argument block, `this`, or a reference to state the loop writes
// leaves that object in memory until the inliner has run, and the kernels
// then compile to other code with other register and spill counts
// ("The sub-minor loops' shared pieces", lists what that kept out
// of here: the stop decision, the phase clock, the next component, the
// record exchange, the general per-thread best and the owner's update stay
// spelled out per kernel).
#pragma once
#include "subminor_internal.h"

namespace rdl {

// ------------------------------------------------------------ all kernels
// Component t of this launch went to pixel (x, y) (LoopArgs::trace,
// trace_cap). The caller decides which thread traces.
__device__ __forceinline__ void WriteTrace(uint32_t* trace, uint64_t trace_cap, uint64_t t,
                                           uint32_t x, uint32_t y) {
  if (t < trace_cap) {
    trace[2 * t] = x;
    trace[2 * t + 1] = y;
  }
}

// LoopArgs::result as the LoopResult
__device__ __forceinline__ void WriteResult(uint32_t* result, uint64_t iteration, float m,
                                            bool diverging, float flux) {
  LoopResult* r = reinterpret_cast<LoopResult*>(result);
  r->iteration = iteration;
  r->peak = m;
  r->diverging = diverging ? 1 : 0;
  r->flux = flux;
}

// ----------------------------------------------------------- Tab and TabN
// The lexicographic (hi, lo) maximum over the active ones of lanes
// 0..LANES-1 (lanes beyond LANES inactive): a DPP max of the high word, one
// ballot, and only on an exact tie a DPP max of the low word. When every
// high word is 0 and the low words of such entries are 0 too (ThreadBest's
// ~bj, a key-0 wave's slot, a key-0 participant's record), every active lane
// ties and lane 0 comes out: the key-0 rule needs no test of its own.
struct LaneWinner {
  int lane;
  uint32_t hi;
};
template <int LANES>
__device__ __forceinline__ LaneWinner LexMaxLane(uint32_t hi, uint32_t lo, bool active) {
  const uint32_t mh = MaxU32<LANES>(active ? hi : 0u);
  const bool mine = active && hi == mh;
  const uint64_t tie = __ballot(mine);
  if ((tie & (tie - 1ull)) == 0ull) return {__builtin_ctzll(tie), mh};
  const uint32_t ml = MaxU32<LANES>(mine ? lo : 0u);
  return {FirstLane(mine && lo == ml), mh};
}

// This thread's best of values[i] (selection index base + tid + i THREADS)
// by |value|, the allow_negative form: the largest key (MaxKey's high word;
// NaN 0, index 0's NaN ~0) by a float max chain (the max skips NaN), then
// the lowest item holding it; compares and selects only, no branch per item.
// bv: the value's bits (values[0]'s when no key is above 0), li: its item.
// (The general form, for allow_negative = 0, stays in the kernels: from here
// it cost them SGPR spills and up to 127 instructions.)
struct ThreadWinner {
  uint32_t bh, bj, bv, li;
};
template <int ITEMS, int THREADS>
__device__ __forceinline__ ThreadWinner ThreadBestAbs(const float (&values)[ITEMS],
                                                      uint32_t base, uint32_t tid,
                                                      uint32_t cnt) {
  uint32_t bj = 0xffffffffu, bv = __float_as_uint(values[0]), li = 0u;
  float tb = -1.0f;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) tb = __builtin_fmaxf(tb, __builtin_fabsf(values[i]));
  uint32_t bh = tb >= 0.0f ? (__float_as_uint(tb) | 0x80000000u) : 0u;
#pragma unroll
  for (int i = ITEMS - 1; i >= 0; --i) {
    const bool eq = __builtin_fabsf(values[i]) == tb;
    bj = eq ? base + tid + uint32_t(i) * THREADS : bj;
    bv = eq ? __float_as_uint(values[i]) : bv;
    li = eq ? uint32_t(i) : li;
  }
  if (base == 0u && tid == 0u && cnt > 0u && values[0] != values[0]) {
    bh = 0xffffffffu;  // selection index 0 holding NaN outranks every key
    bj = 0u;
    li = 0u;
  }
  return {bh, bj, bv, li};
}

// The "fast" exchange of the table kernels publishes records with
// workgroup-scope stores that the other participants poll with agent-scope (L1-bypassing) loads:
// visible to them only because gfx950's vector L1 is write-through, so every
// store reaches the XCD's L2 the participants share (checked at run time:
// all participants on one XCC). A target whose L1 could hold such stores
// needs the agent-scope form, which RDL_SUBMINOR_EXCHANGE=agent selects (and
// tests/test_gpu_kernels.py compares with the fast one).
// Other targets always take the agent-scope form (kFastExchange false).
#if defined(__gfx950__) || !defined(__HIP_DEVICE_COMPILE__)
constexpr bool kFastExchange = true;
#else
constexpr bool kFastExchange = false;
#endif

__device__ __forceinline__ uint32_t XccId() {
  // HW_REG_XCC_ID (hwreg 20), bits [3:0]
  return uint32_t(__builtin_amdgcn_s_getreg((20) | (0 << 6) | ((4 - 1) << 11)));
}

// The G participants exchange their XCC ids through gran[0..G) (zeroed per
// launch; agent-scope stores and loads, whatever the placement). fast: the
// records may go the fast way (every participant on one XCC and no
// agent_exchange); failed: the spin limit was reached.
struct Handshake {
  bool fast, failed;
};
__device__ __forceinline__ Handshake XccHandshake(uint64_t* gran, uint32_t G, uint32_t rank,
                                                  uint32_t lane, uint32_t tid,
                                                  bool agent_exchange) {
  if (tid == 0)
    __hip_atomic_store(gran + rank, (uint64_t(1) << 32) | XccId(), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  uint32_t xcc = 0u;
  bool failed = false;
  for (uint64_t spins = 0; !failed; ++spins) {
    uint64_t v = 0;
    if (lane < G) v = __hip_atomic_load(gran + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__all(lane >= G || (v >> 32) == 1u)) {
      xcc = uint32_t(v);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
    failed = spins > (uint64_t(1) << 24);
  }
  const uint32_t x0 = uint32_t(__builtin_amdgcn_readlane(int(xcc), 0));
  return {kFastExchange && __all(lane >= G || xcc == x0) && !agent_exchange, failed};
}

}  // namespace rdl
