// SubminorLoopReg: the sub-minor loop with each thread's ITEMS selected pixels
// (positions, residuals, model values) held in VGPRs, so one iteration is
//   * ITEMS x N_img PSF gathers issued back to back (one memory round trip),
//   * FMAs + integration + per-thread argmax in registers,
//   * a wave argmax, the wave winner's payload into a parity slot in LDS,
//   * ONE workgroup barrier; every wave then reduces the slots itself.
// With G > 1 workgroups the block winners are exchanged through epoch-tagged
// 8-byte granules ({epoch, word}, single-copy-atomic sc1 stores/loads): wave 0
// sweeps all G records until every tag matches, so the data is the flag and
// no counter or fence round trip is needed (parity-double-buffered so a fast
// block never overwrites a record a slow one has not read).
// From subminor_loop_shared.h: WriteTrace and WriteResult.
#include <type_traits>

#include "subminor_loop_shared.h"

namespace rdl {

template <int NI>
struct RegSlot {
  uint64_t key;
  uint32_t pos;
  float r[NI];
};

__device__ __forceinline__ void StoreGranule(uint64_t* g, uint32_t epoch,
                                             uint32_t v) {
  __hip_atomic_store(g, (uint64_t(epoch) << 32) | v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t LoadGranule(uint64_t* g) {
  return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// IntegratePixel over NI register-resident values, with every per-image
// decision (weight zero, polarization joined, i % n_pol) made once per
// launch: the same floating-point operations in the same order as
// IntegratePixel (rdl_internal.h), without its per-pixel index arithmetic
// and runtime-indexed weight reads.
template <int NI>
struct RegIntegration {
  uint32_t mode = 0, copy = 0, n_img = 0, n_ch = 0, np = 1;
  uint32_t incl = 0;     // LINEAR / SQUARED_JOINS: image k enters the sum
  uint32_t ch_live = 0;  // SQUARE, > 1 channel: channel ch has weight != 0
  uint32_t pol_mask = 0;
  float w[NI];           // weight of image k (SQUARE > 1 ch: of channel k)
  float factor = 1.0f;

  __device__ void Init(const rdl_integration& g) {
    mode = g.mode;
    copy = g.copy_fast_path;
    n_img = g.n_images;
    n_ch = g.n_channels;
    np = g.n_pol;
    pol_mask = g.pol_mask;
    factor = g.factor;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      w[k] = 0.0f;
      if (uint32_t(k) < n_img && mode != RDL_INTEGRATE_SQUARE) {
        w[k] = g.weights[k];
        if (w[k] != 0.0f && ((pol_mask >> (uint32_t(k) % np)) & 1u)) incl |= 1u << k;
      }
      if (mode == RDL_INTEGRATE_SQUARE && uint32_t(k) < n_ch && uint32_t(k) * np < n_img) {
        w[k] = g.weights[uint32_t(k) * np];
        if (w[k] != 0.0f) ch_live |= 1u << k;
      }
    }
  }

  __device__ float operator()(const float (&v)[NI]) const {
    if (copy) return v[0];
    if (mode == RDL_INTEGRATE_LINEAR) {
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
    if (mode == RDL_INTEGRATE_SQUARE) {
      if (n_ch == 1) {
        float acc = 0.0f;
        bool first = true;
#pragma unroll
        for (int p = 0; p < NI; ++p)
          if (uint32_t(p) < np && ((pol_mask >> p) & 1u)) {
            acc = first ? v[p] * v[p] : __builtin_fmaf(v[p], v[p], acc);
            first = false;
          }
        return __builtin_sqrtf(acc) * factor;
      }
      float dest = 0.0f;
#pragma unroll
      for (int ch = 0; ch < NI; ++ch) {
        if (uint32_t(ch) >= n_ch) continue;
        float scratch = 0.0f;
        if ((ch_live >> ch) & 1u) {
          if (np == 1) {
            scratch = v[ch];
          } else {
            float acc = 0.0f;
            bool first = true;
#pragma unroll
            for (int q = 0; q < NI; ++q) {
              const uint32_t p = uint32_t(q) - uint32_t(ch) * np;  // image q = ch np + p
              if (uint32_t(q) >= uint32_t(ch) * np && p < np && ((pol_mask >> p) & 1u)) {
                acc = first ? v[q] * v[q] : __builtin_fmaf(v[q], v[q], acc);
                first = false;
              }
            }
            scratch = first ? 0.0f : __builtin_sqrtf(acc);
          }
        }
        dest = ch == 0 ? scratch * w[ch] : __builtin_fmaf(scratch, w[ch], dest);
      }
      return dest * factor;
    }
    float acc = 0.0f;  // RDL_INTEGRATE_SQUARED_JOINS
    bool first = true;
#pragma unroll
    for (int k = 0; k < NI; ++k)
      if ((incl >> k) & 1u) {
        acc = first ? v[k] * v[k] * w[k] : __builtin_fmaf(v[k] * v[k], w[k], acc);
        first = false;
      }
    return first ? 0.0f : __builtin_sqrtf(acc) * factor;
  }
};

// FAST: one image whose integration is the identity (ImageSet copy fast path,
// cpp/image_set.cc:425-430): the integrated value is the residual itself.
// THREADS = 512 (eight waves, one LDS barrier per iteration) or 64: the
// single-wave form for small selections, where the winner goes from the
// wave argmax straight to every lane by readlane (no LDS slot, no barrier).
template <int NI, int ITEMS, bool FAST, int THREADS = kRegThreads>
__global__ __launch_bounds__(THREADS) void SubminorLoopReg(LoopArgs a) {
  constexpr int REC = 3 + NI;  // granules per record: key hi, key lo, pos, r[NI]
  constexpr int WAVES = THREADS / 64;
  __shared__ RegSlot<NI> slots[2][WAVES];
  __shared__ RegSlot<NI> gwin;
  __shared__ uint32_t gflag;

  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t base = uint64_t(blockIdx.x) * a.per_block;
  const uint32_t cnt =
      base >= a.n_sel ? 0u : uint32_t(min<uint64_t>(a.per_block, a.n_sel - base));
  const int n_img = int(a.n_img);
  const int n_pol = int(a.n_pol);
  RegIntegration<NI> ri;
  if constexpr (!FAST) ri.Init(a.integ);

  uint32_t pos[ITEMS];
  float R[ITEMS][NI];
  float M[ITEMS][NI];
  float F[ITEMS];  // RMS factor of each pixel (1 without one)
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const uint32_t j = tid + uint32_t(i) * THREADS;
    const bool valid = j < cnt;
    pos[i] = valid ? a.pos[base + j] : 0u;
    F[i] = (valid && a.rms)
               ? a.rms[size_t(pos[i] >> 16) * a.width + (pos[i] & 0xffffu)]
               : 1.0f;
#pragma unroll
    for (int k = 0; k < NI; ++k) {
      R[i][k] = (valid && k < n_img) ? a.r[size_t(k) * a.n_sel + base + j] : 0.0f;
      M[i][k] = 0.0f;
    }
  }

  const int W = int(a.width), H = int(a.height);
  const size_t plane = size_t(a.width) * a.height;
  float c[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) c[k] = 0.0f;
  uint32_t cp = 0;  // the component's selection index (its table row)
  int cx = 0, cy = 0;
  bool have_component = false;
  float start_abs = 0.0f;
  bool diverging = false;
  float flux = 0.0f;
  uint64_t iteration = a.iteration_start;
  float m = 0.0f;
  uint32_t epoch = 0;
  uint64_t* gran = reinterpret_cast<uint64_t*>(a.records);

  uint64_t ph[6] = {0, 0, 0, 0, 0, 0};
  const bool prof = a.prof && blockIdx.x == 0 && wave == 0;
  uint64_t t_prev = prof ? __builtin_amdgcn_s_memtime() : 0;
#define RDL_PHASE(i)                                       \
  if (prof) {                                              \
    const uint64_t t_now = __builtin_amdgcn_s_memtime();   \
    ph[i] += t_now - t_prev;                               \
    t_prev = t_now;                                        \
  }
  while (true) {
    // ---- subtract the current component: all gathers first, then FMAs
    if (have_component) {
      float pv[ITEMS][NI];
      bool in[ITEMS];
      if (a.table) {
        // the component's row of the pairwise table: contiguous over j
        const size_t sq = size_t(a.n_sel) * a.n_sel;
        const float* row = a.table + size_t(cp) * a.n_sel + base;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
          const uint32_t j = tid + uint32_t(i) * THREADS;
          const bool valid = j < cnt;
#pragma unroll
          for (int k = 0; k < NI; ++k)
            pv[i][k] = (valid && k < n_img) ? row[size_t(k / n_pol) * sq + j] : 0.0f;
          in[i] = valid && __float_as_uint(pv[i][0]) != kOutsideBits;
        }
      } else {
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const uint32_t j = tid + uint32_t(i) * THREADS;
        const int px = int(pos[i] & 0xffffu), py = int(pos[i] >> 16);
        const int dx = px - cx + W / 2, dy = py - cy + H / 2;
        in[i] = j < cnt && dx >= 0 && dx < W && dy >= 0 && dy < H;
        const size_t off = in[i] ? size_t(dy) * a.width + size_t(dx) : 0;
#pragma unroll
        for (int k = 0; k < NI; ++k)
          pv[i][k] = k < n_img ? a.psfs[size_t(k / n_pol) * plane + off] : 0.0f;
      }
      }
#pragma unroll
      for (int i = 0; i < ITEMS; ++i)
#pragma unroll
        for (int k = 0; k < NI; ++k)
          if (in[i] && k < n_img) R[i][k] = __builtin_fmaf(-pv[i][k], c[k], R[i][k]);
    }
    RDL_PHASE(0)
    // ---- integrate + per-thread argmax
    uint64_t best = 0;
    int best_i = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const uint32_t j = tid + uint32_t(i) * THREADS;
      if (j < cnt) {
        float integ = FAST ? R[i][0] : ri(R[i]);
        if (a.rms) integ *= F[i];  // scratch *= rms (subminor_loop.cc:16-18)
        uint64_t key = MaxKey(integ, a.allow_negative, base + j);
        if (base + j == 0 && integ != integ) key = ~0ull;  // scratch[0] is NaN
        if (key > best) {
          best = key;
          best_i = i;
        }
      }
    }
    // ---- wave argmax; the owner (or lane 0 when nothing qualifies, which
    // stands for selection index 0) writes the wave's slot
    RDL_PHASE(1)
    int owner_lane;
    const uint64_t wmax = KeyMax<64>(best, owner_lane);
    const uint32_t par = epoch & 1u;
    uint64_t gkey;
    uint32_t wpos;
    float wr[NI];
    if constexpr (WAVES == 1) {
      // every lane stages its own candidate; the owner's comes by readlane
      uint32_t pp = pos[0];
      float rr[NI];
#pragma unroll
      for (int k = 0; k < NI; ++k) rr[k] = R[0][k];
#pragma unroll
      for (int i = 1; i < ITEMS; ++i)
        if (i == best_i && wmax != 0) {
          pp = pos[i];
#pragma unroll
          for (int k = 0; k < NI; ++k) rr[k] = R[i][k];
        }
      gkey = wmax;
      wpos = uint32_t(__builtin_amdgcn_readlane(int(pp), owner_lane));
#pragma unroll
      for (int k = 0; k < NI; ++k)
        wr[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rr[k]), owner_lane));
      ++epoch;
      RDL_PHASE(2)
      RDL_PHASE(3)
    } else {
    if (int(lane) == owner_lane) {
      RegSlot<NI>& sl = slots[par][wave];
      sl.key = wmax;
      uint32_t pp = pos[0];
      float rr[NI];
#pragma unroll
      for (int k = 0; k < NI; ++k) rr[k] = R[0][k];
#pragma unroll
      for (int i = 1; i < ITEMS; ++i)
        if (i == best_i && wmax != 0) {
          pp = pos[i];
#pragma unroll
          for (int k = 0; k < NI; ++k) rr[k] = R[i][k];
        }
      sl.pos = pp;
#pragma unroll
      for (int k = 0; k < NI; ++k) sl.r[k] = rr[k];
    }
    RDL_PHASE(2)
    LdsBarrier();
    RDL_PHASE(3)
    // ---- block winner: every wave reduces the slots (ties -> lowest wave,
    // which only matters for the all-zero case)
    // lanes 0..7 read a whole slot each (one LDS round trip); the winner's
    // payload then comes from its lane by readlane
    uint64_t sk = 0ull;
    uint32_t spos = 0;
    float sr[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) sr[k] = 0.0f;
    if (lane < uint32_t(WAVES)) {
      const RegSlot<NI>& sl = slots[par][lane];
      sk = sl.key;
      spos = sl.pos;
#pragma unroll
      for (int k = 0; k < NI; ++k) sr[k] = sl.r[k];
    }
    int bw;
    const uint64_t bkey = KeyMax<(WAVES <= 8 ? 8 : 16)>(sk, bw);
    gkey = bkey;
    wpos = uint32_t(__builtin_amdgcn_readlane(int(spos), bw));
#pragma unroll
    for (int k = 0; k < NI; ++k)
      wr[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sr[k]), bw));

    if (a.n_blocks > 1) {
      ++epoch;  // 1, 2, ... (never 0: granules are zeroed per launch)
      uint64_t* mine = gran + (size_t(par) * a.n_blocks + blockIdx.x) * REC;
      // wave 1 publishes (its stores drain off wave 0's vmcnt) while wave 0
      // sweeps
      if (wave == 1 && lane < uint32_t(REC)) {
        uint32_t v;
        if (lane == 0) v = uint32_t(gkey >> 32);
        else if (lane == 1) v = uint32_t(gkey);
        else if (lane == 2) v = wpos;
        else {
          v = __float_as_uint(wr[0]);
#pragma unroll
          for (int k = 1; k < NI; ++k)
            if (int(lane) - 3 == k) v = __float_as_uint(wr[k]);
        }
        StoreGranule(mine + lane, epoch, v);
      }
      if (wave == 0) {
        // sweep: lane b handles blocks b, b+64, ...; all tags must match
        const uint32_t nb = a.n_blocks;
        uint64_t lk = 0;
        uint32_t lb = 0xffffffffu;
        uint32_t lrec[REC] = {};
        uint64_t spins = 0;
        bool failed = false;
        while (true) {
          bool ok = true;
          lk = 0;
          lb = 0xffffffffu;
          for (uint32_t b = lane; b < nb; b += 64) {
            uint64_t* rec = gran + (size_t(par) * nb + b) * REC;
            uint32_t v[REC];
#pragma unroll
            for (int w = 0; w < REC; ++w) {
              const uint64_t x = LoadGranule(rec + w);
              ok &= uint32_t(x >> 32) == epoch;
              v[w] = uint32_t(x);
            }
            const uint64_t key = (uint64_t(v[0]) << 32) | v[1];
            if (lb == 0xffffffffu || key > lk) {
              lk = key;
              lb = b;
#pragma unroll
              for (int w = 0; w < REC; ++w) lrec[w] = v[w];
            }
          }
          if (__all(ok)) break;
          __builtin_amdgcn_s_sleep(1);
          if (++spins > (uint64_t(1) << 26)) {
            failed = true;
            break;
          }
        }
        // wave argmax over (key, block): keys are unique unless 0, and 0
        // means block 0 (lane 0 holds it first)
        const uint64_t kmax = Max64U64(lk);
        const int src = kmax != 0 ? FirstLane(lk == kmax) : 0;
        uint32_t rec[REC];
#pragma unroll
        for (int w = 0; w < REC; ++w)
          rec[w] = uint32_t(__builtin_amdgcn_readlane(int(lrec[w]), src));
        if (lane == 0) {
          gwin.key = (uint64_t(rec[0]) << 32) | rec[1];
          gwin.pos = rec[2];
#pragma unroll
          for (int kk = 0; kk < NI; ++kk) gwin.r[kk] = __uint_as_float(rec[3 + kk]);
          gflag = failed ? 1u : 0u;
        }
      }
      LdsBarrier();
      if (gflag) {
        if (tid == 0) StoreSc1(&a.result[8], 1u);
        return;
      }
      gkey = gwin.key;
      wpos = gwin.pos;
#pragma unroll
      for (int k = 0; k < NI; ++k) wr[k] = gwin.r[k];
    } else {
      ++epoch;
    }
    }  // WAVES > 1

    RDL_PHASE(4)
    // ---- identical decisions everywhere (subminor_loop.cc:56-89)
    const uint64_t winner_p = (gkey == 0 || gkey == ~0ull)
                                  ? 0ull
                                  : uint64_t(0xffffffffu - uint32_t(gkey));
    m = FAST ? wr[0] : ri(wr);
    if (a.rms) {
      // the winner's integrated x factor is the value its key was made from
      // (with its sign from the integrated value, the factor being >= 0)
      const float kv = KeyValue(gkey);
      m = (gkey == 0 || gkey == ~0ull) ? __int_as_float(0x7fc00000)
          : a.allow_negative            ? copysignf(kv, m)
                                        : kv;
    }
    if (!have_component) {
      start_abs = fabsf(m);
    } else {
      if (a.divergence_limit != 0.0f)
        diverging = fabsf(m) > start_abs * a.divergence_limit;
      ++iteration;
    }
    const bool go = fabsf(m) > a.threshold && iteration < a.max_iterations &&
                    (!a.stop_on_negative || m >= 0.0f) && !diverging;
    if (!go) break;
    if (a.spectral) {
      // PerformSpectralFit of the gain-scaled values (subminor_loop.cc:66-76)
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        float acc = 0.0f;
#pragma unroll
        for (int q = 0; q < NI; ++q)
          if (k < n_img && q < n_img)
            acc = __builtin_fmaf(a.spectral[k * n_img + q], wr[q] * a.gain, acc);
        c[k] = acc;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NI; ++k) c[k] = k < n_img ? wr[k] * a.gain : 0.0f;
    }
    flux += m * a.gain;
    cx = int(wpos & 0xffffu);
    cy = int(wpos >> 16);
    cp = uint32_t(winner_p);
    if (winner_p >= base && winner_p < base + cnt) {
      const uint32_t j = uint32_t(winner_p - base);
      if (j % THREADS == tid) {
        const int wi = int(j / THREADS);
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
          if (i == wi)
#pragma unroll
            for (int k = 0; k < NI; ++k) M[i][k] += c[k];
      }
    }
    if (blockIdx.x == 0 && tid == 0 && a.trace)
      WriteTrace(a.trace, a.trace_cap, iteration - a.iteration_start, uint32_t(cx),
                 uint32_t(cy));
    have_component = true;
    RDL_PHASE(5)
  }
#undef RDL_PHASE
  if (prof && lane == 0) {
    uint64_t* out = reinterpret_cast<uint64_t*>(a.result + 16);
    for (int i = 0; i < 6; ++i) out[i] = ph[i];
  }

#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const uint32_t j = tid + uint32_t(i) * THREADS;
    if (j < cnt)
#pragma unroll
      for (int k = 0; k < NI; ++k)
        if (k < n_img) a.m[size_t(k) * a.n_sel + base + j] = M[i][k];
  }
  if (blockIdx.x == 0 && tid == 0) WriteResult(a.result, iteration, m, diverging, flux);
}

// THREADS = 64: the single wave; 512; 1024: one sixteen-wave workgroup (or a
// grid of them), for selections too large for one 512-thread workgroup's
// registers that would otherwise pay the cross-workgroup exchange every
// iteration.
template <int NI, int ITEMS, int THREADS>
int LaunchReg(const LoopArgs& a, hipStream_t stream) {
  auto kernel = (NI == 1 && a.integ.copy_fast_path)
                    ? SubminorLoopReg<NI, ITEMS, NI == 1, THREADS>
                    : SubminorLoopReg<NI, ITEMS, false, THREADS>;
  return LaunchLoopKernel(kernel, a.n_blocks, THREADS, 0, a, stream);
}

template <int NI>
int LaunchWaveItems(const LoopArgs& a, uint32_t items, hipStream_t stream) {
  constexpr uint32_t kMax = WaveMaxItems(NI);
  if (items <= 1) return LaunchReg<NI, 1, 64>(a, stream);
  if (items <= 2) return LaunchReg<NI, 2, 64>(a, stream);
  if (items <= 4 || kMax <= 4) return LaunchReg<NI, (kMax >= 4 ? 4 : 2), 64>(a, stream);
  if (items <= 8 || kMax <= 8) return LaunchReg<NI, (kMax >= 8 ? 8 : 2), 64>(a, stream);
  return LaunchReg<NI, (kMax >= 16 ? 16 : 2), 64>(a, stream);
}

template <int NI>
int LaunchBigItems(const LoopArgs& a, uint32_t items, hipStream_t stream) {
  if (items <= 1) return LaunchReg<NI, 1, 1024>(a, stream);
  if (items <= 2) return LaunchReg<NI, 2, 1024>(a, stream);
  if (items <= 4 || NI > 2) return LaunchReg<NI, 4, 1024>(a, stream);
  return LaunchReg<NI, 8, 1024>(a, stream);
}

template <int NI>
int LaunchRegItems(const LoopArgs& a, uint32_t items, hipStream_t stream) {
  constexpr uint32_t kMax = RegMaxItems(NI);
  if (items <= 1) return LaunchReg<NI, 1, kRegThreads>(a, stream);
  if (items <= 2 || kMax == 2) return LaunchReg<NI, 2, kRegThreads>(a, stream);
  if (items <= 4 || kMax == 4) return LaunchReg<NI, (kMax >= 4 ? 4 : 2), kRegThreads>(a, stream);
  return LaunchReg<NI, (kMax >= 8 ? 8 : 2), kRegThreads>(a, stream);
}

// f(std::integral_constant<int, NI>) for the register kernels' NI
template <typename F>
int WithNi(uint32_t ni_template, F f) {
  switch (ni_template) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

int LaunchRegLoop(const LoopArgs& a, const LoopPlan& plan, hipStream_t stream) {
  return WithNi(plan.ni_template, [&](auto ni) {
    constexpr int NI = decltype(ni)::value;
    return plan.kind == LoopKind::Big    ? LaunchBigItems<NI>(a, plan.items, stream)
           : plan.kind == LoopKind::Wave ? LaunchWaveItems<NI>(a, plan.items, stream)
                                         : LaunchRegItems<NI>(a, plan.items, stream);
  });
}

}  // namespace rdl
