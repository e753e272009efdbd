// The sub-minor loops that read the pairwise PSF table, and the table's
// builder: SubminorLoopTab (one image, the multiscale hot path) and
// SubminorLoopTabN (joined images). From subminor_loop_shared.h: the
// per-thread best by |value| (ThreadBestAbs), the (hi, lo) winner among lanes
// (LexMaxLane), the participants' handshake (XccHandshake, with the note on
// why the fast exchange is sound), WriteTrace and WriteResult.
#include "subminor_loop_shared.h"

namespace rdl {

// ------------------------------------------------- pairwise PSF table
// table[q][p][j] = PSF q at the offset of selected pixel j from selected
// pixel p (the value the loop gathers for pixel j when p is the component),
// or kOutsideBits where that offset leaves the PSF plane (no subtraction,
// subminor_loop.cc:100-106). Built once per loop by the whole GPU; the loop
// then reads ONE contiguous row per component (coalesced, L2-reusable when a
// component repeats) instead of n_sel scattered gathers.
__global__ __launch_bounds__(256) void BuildPairTable(const uint32_t* __restrict__ pos,
                                                      const float* __restrict__ psfs,
                                                      uint32_t n_sel, uint32_t n_psf,
                                                      uint32_t width, uint32_t height,
                                                      float* __restrict__ table,
                                                      uint64_t* __restrict__ zero,
                                                      uint32_t zero_words) {
  // the loop's per-launch exchange area, zeroed here (no memset launch: the
  // loop runs after this kernel on the same stream)
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (uint32_t w = threadIdx.x; w < zero_words; w += 256) zero[w] = 0ull;
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  const uint32_t p = blockIdx.y;
  if (j >= n_sel) return;
  const uint32_t pp = pos[p], pj = pos[j];
  const int dx = int(pj & 0xffffu) - int(pp & 0xffffu) + int(width / 2);
  const int dy = int(pj >> 16) - int(pp >> 16) + int(height / 2);
  const bool in = dx >= 0 && dx < int(width) && dy >= 0 && dy < int(height);
  const size_t plane = size_t(width) * height;
  const size_t off = in ? size_t(dy) * width + size_t(dx) : 0;
  for (uint32_t q = 0; q < n_psf; ++q)
    table[(size_t(q) * n_sel + p) * n_sel + j] =
        in ? psfs[size_t(q) * plane + off] : __uint_as_float(kOutsideBits);
}

// ------------------------------------------------- pairwise-table loop
// SubminorLoopTab: SubminorLoopReg<1, ITEMS, true, THREADS> specialised for
// the multiscale hot path's common shape — one image whose integration is the
// identity, the pairwise PSF table, no RMS factor, spectral map or
// log-polynomial fit — with the per-iteration dependency chain cut to: the
// table row's loads, FMAs and 32-bit value keys, a DPP wave max whose owner
// is found by one ballot per item (the lowest selection index among equal
// values, as the 64-bit keys order them), one 16-byte LDS slot per wave and
// one LDS barrier, an 8/16-lane DPP max of the slots, scalar decisions.
//
// G > 1 participants split the selection; their block winners are exchanged
// through epoch-tagged 8-byte granules {epoch, word} every wave polls. The
// grid is launched as 8 G blocks of which blocks 0, 8, 16, ... participate
// (one XCD under the dispatcher's round-robin dealing; speed only): the
// participants first exchange their HW_REG_XCC_ID through the placement-
// independent protocol (sc1 stores and sc1 loads) and, only when all of them
// are on one XCD, exchange through that XCD's L2 (plain stores, which keep
// the line in L2, polled by sc1 loads, which bypass only L1); otherwise every
// granule goes through sc1 stores as well. RDL_TRACE_SUBMINOR=1 measured the
// sc1 exchange at ~4 700 of ~7 800 cycles per iteration.
//
// Same operations in the same order, same argmax order and tie rules as the
// generic kernels: traces and model values are identical.
template <int ITEMS, int THREADS, bool NEG>
__global__ __launch_bounds__(THREADS) void SubminorLoopTab(LoopArgs a) {
  constexpr int WAVES = THREADS / 64;
  constexpr int SLANES = WAVES <= 8 ? 8 : 16;
  // {key hi, key lo, value bits, -}, parity double-buffered
  __shared__ uint4 slots[2][WAVES];
  // the atomic form (G == 1): per iteration one 64-bit key cell and the
  // bits of selection index 0's value, triple-buffered (a cell is cleared
  // two iterations before its next use, after a barrier every reader of
  // its last use has passed)
  __shared__ unsigned long long cells[3];
  __shared__ uint32_t first_bits[3];
  const uint32_t G = a.n_blocks;
  if (G > 1 && blockIdx.x % a.part_stride != 0u) return;
  const uint32_t rank = G > 1 ? blockIdx.x / a.part_stride : 0u;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = uint32_t(a.n_sel), per = a.per_block;
  const uint32_t base = rank * per;
  const uint32_t cnt = base >= n ? 0u : min(per, n - base);
  const bool neg = a.allow_negative != 0;
  // exchange granules (zeroed per launch): [G] XCC ids, then [2][G][3] records
  uint64_t* gran = reinterpret_cast<uint64_t*>(a.records);
  uint64_t* recs = gran + G;
  float R[ITEMS], M[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const uint32_t j = tid + uint32_t(i) * THREADS;
    // beyond the slice: NaN (key 0, never a winner; see the padded table)
    R[i] = j < cnt ? a.r[base + j] : __int_as_float(0x7fc00000);
    M[i] = 0.0f;
  }
  bool fast = true;  // G > 1: exchange through the one L2 of the participants
  bool failed = false;
  if (G > 1) {
    const Handshake hs = XccHandshake(gran, G, rank, lane, tid, a.agent_exchange != 0);
    fast = hs.fast;
    failed = hs.failed;
  }
  const float* table = a.table;
  float c = 0.0f, m = 0.0f, start_abs = 0.0f, flux = 0.0f;
  uint32_t par = 0, epoch = 0;
  uint32_t row_cp = 0xffffffffu;  // the component whose row pv holds
  float pv[ITEMS];
  uint32_t pend_pos = 0;
  bool pend = false;  // a trace entry waiting for its position's load
  bool have = false, diverging = false;
  uint64_t iteration = a.iteration_start;
  const bool tracer = rank == 0 && tid == 0 && a.trace;
  const bool atomic = G == 1 && a.atomic_reduce != 0;
  uint32_t cell = 0;  // iteration % 3
  if (atomic) {
    if (tid < 3u) cells[tid] = 0ull;
    LdsBarrier();
  }
  // the loop's comparisons as integer tests on float bits (see decisions)
  const uint32_t thr_bits = __float_as_uint(a.threshold) & 0x7fffffffu;
  const uint32_t thr_mode = a.threshold != a.threshold        ? 0u
                            : (__float_as_uint(a.threshold) >> 31) && thr_bits ? 1u
                                                                                : 2u;
  uint32_t lim_mode = 0u, lim_bits = 0u;
  const bool stop_neg = a.stop_on_negative != 0;
  uint64_t remaining =
      a.max_iterations > a.iteration_start ? a.max_iterations - a.iteration_start : 0u;
  // RDL_TRACE_SUBMINOR=1: per-phase cycles of participant 0, wave 0
  uint64_t ph[6] = {0, 0, 0, 0, 0, 0};
  const bool prof = a.prof && rank == 0 && wave == 0;
  uint64_t t_prev = prof ? __builtin_amdgcn_s_memtime() : 0;
#define RDL_TPHASE(i)                                      \
  if (prof) {                                              \
    const uint64_t t_now = __builtin_amdgcn_s_memtime();   \
    ph[i] += t_now - t_prev;                               \
    t_prev = t_now;                                        \
  }
  while (!failed) {
    if (have) {
      // the component's row of the pairwise table (contiguous over j), issued
      // before the previous iteration's decisions (a repeated component
      // reuses the row already in registers); the FMAs (subminor_loop.cc:
      // 93-108)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
        if (__float_as_uint(pv[i]) != kOutsideBits) R[i] = __builtin_fmaf(-pv[i], c, R[i]);
      if (pend) {  // the previous component's position has arrived with the row
        WriteTrace(a.trace, a.trace_cap, iteration - a.iteration_start, pend_pos & 0xffffu,
                   pend_pos >> 16);
        pend = false;
      }
    }
    RDL_TPHASE(0)
    // ---- this thread's best: the largest key, then the lowest index
    uint32_t bh = 0u, bj = 0xffffffffu, bv = __float_as_uint(R[0]);
    if constexpr (NEG) {
      const ThreadWinner best = ThreadBestAbs<ITEMS, THREADS>(R, base, tid, cnt);
      bh = best.bh;
      bj = best.bj;
      bv = best.bv;
    } else {
      // the general form (ThreadBestAbs's rule on MaxKey's high word of R or
      // |R|; spelled out here and in SubminorLoopTabN)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const float v = neg ? fabsf(R[i]) : R[i];
        const uint32_t u = __float_as_uint(v);
        uint32_t h = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        const uint32_t j = base + tid + uint32_t(i) * THREADS;
        if (v != v) h = (j == 0u && cnt > 0u) ? 0xffffffffu : 0u;
        const bool better = h > bh;  // items ascend in j: equal keys keep the first
        bh = better ? h : bh;
        bj = better ? j : bj;
        bv = better ? __float_as_uint(R[i]) : bv;
      }
    }
    RDL_TPHASE(1)
    uint32_t gh, gl, gv;
    if (atomic) {
      // ---- block winner: the 64-bit key (value word, then the lowest
      // selection index, then the value's sign bit to rebuild it) as one LDS
      // atomic max per 16-lane row after a DPP max within the row; the same
      // total order as the two-level (hi, ~j) reduction below. A key-0 lane
      // (every item NaN / beyond the slice) holds 0; selection index 0's
      // value bits stand for the all-zero (and the NaN-at-0) outcome.
      uint64_t key = 0ull;
      if (bh != 0u)
        key = (uint64_t(bh) << 32) | (uint64_t((0x7fffffffu - bj) << 1) | (bv >> 31));
      uint64_t t;
      t = DppU64<0xb1>(key);
      key = t > key ? t : key;
      t = DppU64<0x4e>(key);
      key = t > key ? t : key;
      t = DppU64<0x141>(key);
      key = t > key ? t : key;
      t = DppU64<0x140>(key);
      key = t > key ? t : key;
      if ((lane & 15u) == 0u && key != 0ull) atomicMax(&cells[cell], (unsigned long long)key);
      if (tid == 0) first_bits[cell] = __float_as_uint(R[0]);
      RDL_TPHASE(2)
      LdsBarrier();
      RDL_TPHASE(3)
      const uint64_t k = cells[cell];
      const uint32_t fb = first_bits[cell];
      if (tid == 0) cells[cell == 0u ? 2u : cell - 1u] = 0ull;  // used two iterations on
      cell = cell == 2u ? 0u : cell + 1u;
      gh = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(k >> 32))));
      const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(k))));
      const uint32_t fbs = uint32_t(__builtin_amdgcn_readfirstlane(int(fb)));
      const uint32_t j = 0x7fffffffu - (lo >> 1);
      gl = gh == 0u ? 0u : ~j;
      if (gh == 0u || gh == 0xffffffffu) {
        gv = fbs;  // selection index 0's value (all keys 0, or NaN at index 0)
      } else if (NEG || neg) {
        gv = (gh & 0x7fffffffu) | (lo << 31);  // |R| bits, R's sign
      } else {
        gv = (gh & 0x80000000u) ? (gh & 0x7fffffffu) : ~gh;  // the key transform inverted
      }
    } else {
    // ---- wave winner: DPP max of the keys; the lowest index on exact ties
    const LaneWinner ww = LexMaxLane<64>(bh, ~bj, true);
    const uint32_t mh = ww.hi;
    int owner = ww.lane;
    // a key-0 wave stands for its first pixel (lane 0's item 0, as
    // SubminorLoopReg), whose value is lane 0's initial bv
    const uint32_t wl = mh == 0u ? 0u : ~uint32_t(__builtin_amdgcn_readlane(int(bj), owner));
    const uint32_t wv = uint32_t(__builtin_amdgcn_readlane(int(bv), mh == 0u ? 0 : owner));
    if (lane == 0) slots[par][wave] = make_uint4(mh, wl, wv, 0u);
    RDL_TPHASE(2)
    LdsBarrier();
    RDL_TPHASE(3)
    // ---- block winner over the wave slots
    const uint4 s4 = lane < uint32_t(WAVES) ? slots[par][lane] : make_uint4(0u, 0u, 0u, 0u);
    par ^= 1u;
    {
      const LaneWinner bw = LexMaxLane<SLANES>(s4.x, s4.y, lane < uint32_t(WAVES));
      gh = bw.hi;
      owner = bw.lane;
    }
    gl = uint32_t(__builtin_amdgcn_readlane(int(s4.y), owner));
    gv = uint32_t(__builtin_amdgcn_readlane(int(s4.z), owner));
    if (G > 1) {
      // ---- exchange of the participants' winners
      ++epoch;  // 1, 2, ... (granules are zeroed per launch)
      uint64_t* mine_rec = recs + (size_t(epoch & 1u) * G + rank) * 3;
      if (wave == 0 && lane < 3u) {
        const uint32_t w = lane == 0 ? gh : lane == 1 ? gl : gv;
        const uint64_t g = (uint64_t(epoch) << 32) | w;
        if (fast)
          __hip_atomic_store(mine_rec + lane, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
          __hip_atomic_store(mine_rec + lane, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      uint32_t xh = 0u, xl = 0u, xv = 0u;
      for (uint64_t spins = 0;; ++spins) {
        bool ok = true;
        if (lane < G) {
          const uint64_t* rr = recs + (size_t(epoch & 1u) * G + lane) * 3;
          const uint64_t g0 = __hip_atomic_load(rr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t g1 =
              __hip_atomic_load(rr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t g2 =
              __hip_atomic_load(rr + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          ok = uint32_t(g0 >> 32) == epoch && uint32_t(g1 >> 32) == epoch &&
               uint32_t(g2 >> 32) == epoch;
          xh = uint32_t(g0);
          xl = uint32_t(g1);
          xv = uint32_t(g2);
        }
        if (__all(ok)) break;
        if (spins > (uint64_t(1) << 26)) {
          failed = true;
          break;
        }
      }
      if (failed) break;
      // lexicographic (hi, lo) max over the participants (lanes < G)
      const LaneWinner xw = LexMaxLane<64>(xh, xl, lane < G);
      gh = xw.hi;
      const int win = xw.lane;
      gl = uint32_t(__builtin_amdgcn_readlane(int(xl), win));
      gv = uint32_t(__builtin_amdgcn_readlane(int(xv), win));
    }
    }  // the wave-slot reduction
    RDL_TPHASE(4)
    // ---- identical decisions everywhere (subminor_loop.cc:56-89), on the
    // bit patterns in scalar registers (exact: |x| > t for t >= 0 is the
    // integer order of the bits; NaN never passes a comparison)
    const bool none = gh == 0u || (gh == 0xffffffffu && gl == 0xffffffffu);
    const uint32_t wp = none ? 0u : 0xffffffffu - gl;
    // the winner's table row: in flight while the decisions run (a row the
    // loop then does not use is only read; wp < n_sel always)
    if (wp != row_cp) {
      const float* row = table + size_t(wp) * n + base;
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) pv[i] = row[tid + uint32_t(i) * THREADS];
      row_cp = wp;
    }
    m = __uint_as_float(gv);
    const uint32_t ab = gv & 0x7fffffffu;
    const bool is_nan = ab > 0x7f800000u;
    if (!have) {
      start_abs = __uint_as_float(ab);
      if (a.divergence_limit != 0.0f) {
        const float lim = start_abs * a.divergence_limit;
        lim_bits = __float_as_uint(lim) & 0x7fffffffu;
        lim_mode = lim != lim ? 0u : ((__float_as_uint(lim) >> 31) && lim_bits) ? 1u : 2u;
      }
    } else {
      // fabsf(m) > start_abs * divergence_limit
      diverging = lim_mode == 1u ? !is_nan : lim_mode == 2u ? (!is_nan && ab > lim_bits) : false;
      ++iteration;
      --remaining;
    }
    const bool above = thr_mode == 1u ? !is_nan : thr_mode == 2u ? (!is_nan && ab > thr_bits)
                                                               : false;
    // !stop_on_negative || m >= 0 (-0 included, NaN excluded)
    const bool non_negative = !is_nan && ((gv >> 31) == 0u || gv == 0x80000000u);
    const bool go = above && remaining != 0u && (!stop_neg || non_negative) && !diverging;
    if (!go) break;
    c = m * a.gain;
    flux += c;  // flux += m * gain (the same product)
    // the owner lane adds the component (scalar branches to its wave and item)
    {
      const uint32_t off = wp - base;
      if (off < cnt && (off % uint32_t(THREADS)) / 64u == wave) {
        const uint32_t wi = off / uint32_t(THREADS);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
          if (uint32_t(i) == wi && lane == (off & 63u)) M[i] += c;
      }
    }
    if (tracer) {  // the load lands with the next row's (one wait for both)
      pend_pos = a.pos[wp];
      pend = true;
    }
    have = true;
    RDL_TPHASE(5)
  }
#undef RDL_TPHASE
  if (prof && lane == 0) {
    uint64_t* out = reinterpret_cast<uint64_t*>(a.result + 16);
    for (int i = 0; i < 6; ++i) out[i] = ph[i];
  }
  if (pend)
    WriteTrace(a.trace, a.trace_cap, iteration - a.iteration_start, pend_pos & 0xffffu,
               pend_pos >> 16);
  if (failed) {
    if (tid == 0) StoreSc1(&a.result[8], 1u);
    return;
  }
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const uint32_t j = tid + uint32_t(i) * THREADS;
    if (j < cnt) a.m[base + j] = M[i];
  }
  if (rank == 0 && tid == 0) WriteResult(a.result, iteration, m, diverging, flux);
}

// RegIntegration's RDL_INTEGRATE_LINEAR branch alone (SubminorLoopTabN's
// integrations): the same operations in the same order
template <int NI>
struct LinearIntegration {
  uint32_t incl = 0;
  float w[NI];
  float factor = 1.0f;
  __device__ void Init(const rdl_integration& g) {
    factor = g.factor;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      w[k] = uint32_t(k) < g.n_images ? g.weights[k] : 0.0f;
      if (uint32_t(k) < g.n_images && w[k] != 0.0f && ((g.pol_mask >> (uint32_t(k) % g.n_pol)) & 1u))
        incl |= 1u << k;
    }
  }
  __device__ float operator()(const float (&v)[NI]) const {
    float acc = 0.0f;
    bool first = true;
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if ((incl >> k) & 1u) {
        acc = first ? v[k] * w[k] : __builtin_fmaf(v[k], w[k], acc);
        first = false;
      }
    return first ? 0.0f : acc * factor;
  }
};

// ------------------------------------------------- pairwise-table loop, N_img
// SubminorLoopTabN: SubminorLoopTab for joined images (NI = 2..8 images of
// one polarization, each with its own PSF, the linear integration; no RMS
// factor, spectral map or log-polynomial fit). Per iteration the component's table row of
// every PSF (FMAs into the register-resident images), the integrated value
// per pixel, the key argmax as SubminorLoopTab's (|integrated| max chain with
// allow_negative), the wave winner's image values through its LDS slot, and
// for G > 1 participants (one XCD, as SubminorLoopTab) records of 3 + N_img
// epoch-tagged granules. The same operations in the same order as
// SubminorLoopReg: traces and model values are identical.
template <int NI, int ITEMS, int THREADS, bool NEG>
__global__ __launch_bounds__(THREADS) void SubminorLoopTabN(LoopArgs a) {
  constexpr int WAVES = THREADS / 64;
  constexpr int SLANES = WAVES <= 8 ? 8 : 16;
  constexpr uint32_t REC = 3 + NI;
  __shared__ uint4 slots[2][WAVES];     // {key hi, key lo, integrated bits, -}
  __shared__ float slotv[2][WAVES][NI];  // the wave winner's image values
  const uint32_t G = a.n_blocks;
  if (G > 1 && blockIdx.x % a.part_stride != 0u) return;
  const uint32_t rank = G > 1 ? blockIdx.x / a.part_stride : 0u;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = uint32_t(a.n_sel), per = a.per_block;
  const uint32_t base = rank * per;
  const uint32_t cnt = base >= n ? 0u : min(per, n - base);
  const bool neg = a.allow_negative != 0;
  LinearIntegration<NI> ri;
  ri.Init(a.integ);
  // uniform values kept in VGPRs (one wave per SIMD leaves them free; as
  // SGPRs they spilled): weights, factor, and below the component values
#pragma unroll
  for (int k = 0; k < NI; ++k) asm volatile("" : "+v"(ri.w[k]));
  asm volatile("" : "+v"(ri.factor));
  uint64_t* gran = reinterpret_cast<uint64_t*>(a.records);
  uint64_t* recs = gran + G;
  float R[ITEMS][NI], M[ITEMS][NI];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const uint32_t j = tid + uint32_t(i) * THREADS;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      // beyond the slice: NaN (never a winner; see the padded table)
      R[i][k] = j < cnt ? a.r[size_t(k) * n + base + j] : __int_as_float(0x7fc00000);
      M[i][k] = 0.0f;
    }
  }
  bool fast = true;
  bool failed = false;
  if (G > 1) {
    const Handshake hs = XccHandshake(gran, G, rank, lane, tid, a.agent_exchange != 0);
    fast = hs.fast;
    failed = hs.failed;
  }
  const size_t sq = size_t(n) * n;
  float c[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) c[k] = 0.0f;
  float m = 0.0f, start_abs = 0.0f, flux = 0.0f;
  uint32_t par = 0, epoch = 0;
  uint32_t row_cp = 0xffffffffu;
  float pv[ITEMS][NI];
  uint32_t pend_pos = 0;
  bool pend = false, have = false, diverging = false;
  uint64_t iteration = a.iteration_start;
  const bool tracer = rank == 0 && tid == 0 && a.trace;
  const uint32_t thr_bits = __float_as_uint(a.threshold) & 0x7fffffffu;
  const uint32_t thr_mode = a.threshold != a.threshold        ? 0u
                            : (__float_as_uint(a.threshold) >> 31) && thr_bits ? 1u
                                                                                : 2u;
  uint32_t lim_mode = 0u, lim_bits = 0u;
  const bool stop_neg = a.stop_on_negative != 0;
  uint64_t remaining =
      a.max_iterations > a.iteration_start ? a.max_iterations - a.iteration_start : 0u;
  while (!failed) {
    if (have) {
      // the component's row of every PSF (contiguous over j), issued before
      // the previous iteration's decisions
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const bool in = __float_as_uint(pv[i][0]) != kOutsideBits;
#pragma unroll
        for (int k = 0; k < NI; ++k) {
          const float t = __builtin_fmaf(-pv[i][k], c[k], R[i][k]);
          R[i][k] = in ? t : R[i][k];
        }
      }
      if (pend) {
        WriteTrace(a.trace, a.trace_cap, iteration - a.iteration_start, pend_pos & 0xffffu,
                   pend_pos >> 16);
        pend = false;
      }
    }
    // ---- integrated values and this thread's best (as SubminorLoopTab)
    float iv[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) iv[i] = ri(R[i]);
    uint32_t bh = 0u, bj = 0xffffffffu, bv = __float_as_uint(iv[0]), li = 0u;
    if constexpr (NEG) {
      const ThreadWinner best = ThreadBestAbs<ITEMS, THREADS>(iv, base, tid, cnt);
      bh = best.bh;
      bj = best.bj;
      bv = best.bv;
      li = best.li;
    } else {
      // the general form, as SubminorLoopTab's, with the item
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const float v = neg ? fabsf(iv[i]) : iv[i];
        const uint32_t u = __float_as_uint(v);
        uint32_t h = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        const uint32_t j = base + tid + uint32_t(i) * THREADS;
        if (v != v) h = (j == 0u && cnt > 0u) ? 0xffffffffu : 0u;
        const bool better = h > bh;
        bh = better ? h : bh;
        bj = better ? j : bj;
        bv = better ? __float_as_uint(iv[i]) : bv;
        li = better ? uint32_t(i) : li;
      }
    }
    // ---- wave winner and its image values: LexMaxLane<64>(bh, ~bj, true)
    // spelled out (called here, next to ThreadBestAbs, it took one VGPR off four
    // instantiations), with a shortcut for a key-0 wave
    const uint32_t mh = MaxU32<64>(bh);
    const uint64_t tie = __ballot(bh == mh);
    int owner;
    if (mh == 0u) {
      owner = 0;  // a key-0 wave stands for lane 0's item 0
    } else if ((tie & (tie - 1ull)) == 0ull) {
      owner = __builtin_ctzll(tie);
    } else {
      const uint32_t ml = MaxU32<64>(bh == mh ? ~bj : 0u);
      owner = FirstLane(bh == mh && ~bj == ml);
    }
    const uint32_t wl = mh == 0u ? 0u : ~uint32_t(__builtin_amdgcn_readlane(int(bj), owner));
    const uint32_t wv = uint32_t(__builtin_amdgcn_readlane(int(bv), owner));
    if (lane == 0) slots[par][wave] = make_uint4(mh, wl, wv, 0u);
    // the owner lane stores its candidate's image values (a key-0 wave: lane
    // 0's item 0, li = 0)
    if (int(lane) == owner) {
      float v[NI];
#pragma unroll
      for (int k = 0; k < NI; ++k) v[k] = R[0][k];
#pragma unroll
      for (int i = 1; i < ITEMS; ++i)
#pragma unroll
        for (int k = 0; k < NI; ++k) v[k] = li == uint32_t(i) ? R[i][k] : v[k];
#pragma unroll
      for (int k = 0; k < NI; ++k) slotv[par][wave][k] = v[k];
    }
    LdsBarrier();
    // ---- block winner over the wave slots
    const uint4 s4 = lane < uint32_t(WAVES) ? slots[par][lane] : make_uint4(0u, 0u, 0u, 0u);
    const LaneWinner bw = LexMaxLane<SLANES>(s4.x, s4.y, lane < uint32_t(WAVES));
    uint32_t gh = bw.hi;
    owner = bw.lane;
    uint32_t gl = uint32_t(__builtin_amdgcn_readlane(int(s4.y), owner));
    uint32_t gv = uint32_t(__builtin_amdgcn_readlane(int(s4.z), owner));
    float wr[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      wr[k] = slotv[par][owner][k];
      asm volatile("" : "+v"(wr[k]));
    }
    par ^= 1u;
    if (G > 1) {
      ++epoch;
      uint64_t* mine_rec = recs + (size_t(epoch & 1u) * G + rank) * REC;
      if (wave == 0 && lane < REC) {
        uint32_t w = lane == 0 ? gh : lane == 1 ? gl : gv;
#pragma unroll
        for (int k = 0; k < NI; ++k)
          if (lane == 3u + uint32_t(k)) w = __float_as_uint(wr[k]);
        const uint64_t g = (uint64_t(epoch) << 32) | w;
        if (fast)
          __hip_atomic_store(mine_rec + lane, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
          __hip_atomic_store(mine_rec + lane, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      uint32_t xr[REC];
#pragma unroll
      for (uint32_t w = 0; w < REC; ++w) xr[w] = 0u;
      for (uint64_t spins = 0;; ++spins) {
        bool ok = true;
        if (lane < G) {
          const uint64_t* rr = recs + (size_t(epoch & 1u) * G + lane) * REC;
#pragma unroll
          for (uint32_t w = 0; w < REC; ++w) {
            const uint64_t g = __hip_atomic_load(rr + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = ok && uint32_t(g >> 32) == epoch;
            xr[w] = uint32_t(g);
          }
        }
        if (__all(ok)) break;
        if (spins > (uint64_t(1) << 26)) {
          failed = true;
          break;
        }
      }
      if (failed) break;
      const LaneWinner xw = LexMaxLane<64>(xr[0], xr[1], lane < G);
      gh = xw.hi;
      const int win = xw.lane;
      gl = uint32_t(__builtin_amdgcn_readlane(int(xr[1]), win));
      gv = uint32_t(__builtin_amdgcn_readlane(int(xr[2]), win));
#pragma unroll
      for (int k = 0; k < NI; ++k)
        wr[k] = __uint_as_float(uint32_t(__builtin_amdgcn_readlane(int(xr[3 + k]), win)));
    }
    // ---- decisions (as SubminorLoopTab, on the integrated value's bits)
    const bool none = gh == 0u || (gh == 0xffffffffu && gl == 0xffffffffu);
    const uint32_t wp = none ? 0u : 0xffffffffu - gl;
    if (wp != row_cp) {
#pragma unroll
      for (int q = 0; q < NI; ++q) {
        const float* row = a.table + size_t(q) * sq + size_t(wp) * n + base;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) pv[i][q] = row[tid + uint32_t(i) * THREADS];
      }
      row_cp = wp;
    }
    m = __uint_as_float(gv);
    const uint32_t ab = gv & 0x7fffffffu;
    const bool is_nan = ab > 0x7f800000u;
    if (!have) {
      start_abs = __uint_as_float(ab);
      if (a.divergence_limit != 0.0f) {
        const float lim = start_abs * a.divergence_limit;
        lim_bits = __float_as_uint(lim) & 0x7fffffffu;
        lim_mode = lim != lim ? 0u : ((__float_as_uint(lim) >> 31) && lim_bits) ? 1u : 2u;
      }
    } else {
      diverging = lim_mode == 1u ? !is_nan : lim_mode == 2u ? (!is_nan && ab > lim_bits) : false;
      ++iteration;
      --remaining;
    }
    const bool above = thr_mode == 1u ? !is_nan : thr_mode == 2u ? (!is_nan && ab > thr_bits)
                                                               : false;
    const bool non_negative = !is_nan && ((gv >> 31) == 0u || gv == 0x80000000u);
    const bool go = above && remaining != 0u && (!stop_neg || non_negative) && !diverging;
    if (!go) break;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      c[k] = wr[k] * a.gain;
      asm volatile("" : "+v"(c[k]));
    }
    flux += m * a.gain;
    {
      const uint32_t off = wp - base;
      if (off < cnt && (off % uint32_t(THREADS)) / 64u == wave) {
        const uint32_t oi = off / uint32_t(THREADS);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
          if (uint32_t(i) == oi && lane == (off & 63u))
#pragma unroll
            for (int k = 0; k < NI; ++k) M[i][k] += c[k];
      }
    }
    if (tracer) {
      pend_pos = a.pos[wp];
      pend = true;
    }
    have = true;
  }
  if (pend)
    WriteTrace(a.trace, a.trace_cap, iteration - a.iteration_start, pend_pos & 0xffffu,
               pend_pos >> 16);
  if (failed) {
    if (tid == 0) StoreSc1(&a.result[8], 1u);
    return;
  }
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const uint32_t j = tid + uint32_t(i) * THREADS;
    if (j < cnt)
#pragma unroll
      for (int k = 0; k < NI; ++k) a.m[size_t(k) * n + base + j] = M[i][k];
  }
  if (rank == 0 && tid == 0) WriteResult(a.result, iteration, m, diverging, flux);
}

template <int NI, bool NEG>
auto TabNKernel(uint32_t items) {
  return items <= 1   ? SubminorLoopTabN<NI, 1, 256, NEG>
         : items <= 2 ? SubminorLoopTabN<NI, 2, 256, NEG>
                      : SubminorLoopTabN<NI, 4, 256, NEG>;
}

template <int NI>
int LaunchTabN(const LoopArgs& a, uint32_t items, hipStream_t stream) {
  auto k = a.allow_negative ? TabNKernel<NI, true>(items) : TabNKernel<NI, false>(items);
  return LaunchLoopKernel(k, a.n_blocks * a.part_stride, 256, 0, a, stream);
}

template <int THREADS, bool NEG>
auto TabKernel(uint32_t items) {
  return items <= 1    ? SubminorLoopTab<1, THREADS, NEG>
         : items <= 2  ? SubminorLoopTab<2, THREADS, NEG>
         : items <= 4  ? SubminorLoopTab<4, THREADS, NEG>
         : items <= 8  ? SubminorLoopTab<8, THREADS, NEG>
         : items <= 16 ? SubminorLoopTab<16, THREADS, NEG>
                       : SubminorLoopTab<(THREADS <= 256 ? 32 : 16), THREADS, NEG>;
}

template <int THREADS>
int LaunchTab(const LoopArgs& a, uint32_t items, hipStream_t stream) {
  auto k = a.allow_negative ? TabKernel<THREADS, true>(items) : TabKernel<THREADS, false>(items);
  return LaunchLoopKernel(k, a.n_blocks * a.part_stride, THREADS, 0, a, stream);
}

int LaunchTabLoop(const LoopArgs& a, const LoopPlan& plan, hipStream_t stream) {
  if (plan.kind == LoopKind::TabN) {
    switch (a.n_img) {
      case 2: return LaunchTabN<2>(a, plan.items, stream);
      case 3: return LaunchTabN<3>(a, plan.items, stream);
      case 4: return LaunchTabN<4>(a, plan.items, stream);
      case 5: return LaunchTabN<5>(a, plan.items, stream);
      case 6: return LaunchTabN<6>(a, plan.items, stream);
      case 7: return LaunchTabN<7>(a, plan.items, stream);
      default: return LaunchTabN<8>(a, plan.items, stream);
    }
  }
  if (plan.threads == 256) return LaunchTab<256>(a, plan.items, stream);
  if (plan.threads == 512) return LaunchTab<512>(a, plan.items, stream);
  return LaunchTab<1024>(a, plan.items, stream);
}

int LaunchPairTable(const uint32_t* pos, const float* psfs, uint32_t n_sel, uint32_t n_psf,
                    uint32_t width, uint32_t height, float* table, uint64_t* zero,
                    uint32_t zero_words, hipStream_t stream) {
  BuildPairTable<<<dim3(DivUp(n_sel, 256), n_sel), 256, 0, stream>>>(
      pos, psfs, n_sel, n_psf, width, height, table, zero, zero_words);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

}  // namespace rdl
