// The float row plans with their LDS-DMA kernels, and the launchers of every
// row plan (the kernels both precisions share: fft_fast_rows.h).
#include <algorithm>
#include <cstdlib>

#include "fft_fast_rows.h"

namespace rdl {
namespace ff {

// One 16-byte-per-lane LDS-DMA load (global_load_lds_dwordx4): lane i's 16 B
// land at LDS byte `lds` + 16 i (lds wave-uniform, through m0). In inline asm
// so the compiler does not treat it as an LDS write of unknown extent (see
// RowsInverseDma); the caller retires it with its own s_waitcnt vmcnt and a
// barrier before any wave reads those bytes.
__device__ __forceinline__ void DmaLoad16(const void* g, uint32_t lds) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(g), "s"(lds)
      : "memory");
}

// RowsInverse (float, tiled spectrum, write mode, even window) with the next
// row's spectrum fetched by LDS-DMA while this row is transformed and
// stored. The persistent row kernel keeps one row per workgroup in
// flight only while that workgroup loads it (a third of its time at three
// workgroups per CU: ~3 TB/s); here every workgroup always has its next row
// in flight (global_load_lds_dwordx4: a wave instruction moves 8 tiles x
// 128 B, lane-linear into `raw`, no VGPRs), and the FFT runs in its own LDS
// buffer. The DMA is retired by a counted vmcnt (the 16 output stores per
// wave issued after it may stay in flight) and a barrier; every other
// synchronisation is LDS-only, so nothing drains it early. Same arithmetic
// as RowsInverse<float, TH, true> (FftC, zc, the fused peak search).
template <uint32_t TH, uint32_t... Rs>
__global__ __launch_bounds__(TH) void RowsInverseDma(RowArgs a, const Cx<float>* __restrict__ spec,
                                                     float* __restrict__ out,
                                                     const Cx<double>* __restrict__ twd) {
  constexpr uint32_t H = Product<Rs...>();
  constexpr uint32_t EH = H / TH;
  static_assert(H % TH == 0 && (EH == 16 || EH == 8), "vmcnt counts of 8 or 16 stores");
  constexpr uint32_t WAVES = TH / 64;
  constexpr uint32_t ND1 = 2 * H / kTwdLo;
  constexpr uint32_t NT = (H + 1 + kTile - 1) / kTile;  // spectrum tiles per row
  constexpr uint32_t NI = (NT + 7) / 8;                 // DMA wave instructions per row
  typedef __attribute__((address_space(3))) void* LdsPtr;
  // The DMA target is its own __shared__ object; the transform, tables and
  // reduction live in the dynamic array (RowsDmaLdsBytes). The DMA is issued
  // by inline asm (DmaLoad16): hipcc cannot tell which LDS bytes a
  // global_load_lds writes and, for its builtin, waits vmcnt(0) before the
  // next LDS read whatever the arrays, which drained the prefetch at once.
  __shared__ __attribute__((aligned(16))) Cx<float> raw[NI * 8 * kTile];
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr uint32_t NCT = CachedTableSize<1, Rs...>(TH, H);
  Cx<float>* buf = reinterpret_cast<Cx<float>*>(lds_raw);             // the transform
  Cx<double>* tws = reinterpret_cast<Cx<double>*>(buf + (H + (H >> kFastPadShift)));
  Cx<float>* ctab = reinterpret_cast<Cx<float>*>(tws + ND1 + kTwdLo);
  uint64_t* red = reinterpret_cast<uint64_t*>(ctab + (NCT > 0 ? (NCT + 1) / 2 * 2 : 2));
  TwdLds td{tws, tws + ND1};
  Cx<float> clast[LastRadix<Rs...>() - 1];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  auto issue = [&](uint32_t iy) {
    const size_t y = size_t(iy) + a.oy;
    for (uint32_t j = wave; j < NI; j += WAVES) {
      const uint32_t t = j * 8 + lane / 8;
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          uint32_t(uintptr_t((LdsPtr)(raw + j * 8 * kTile))));
      if (t < NT) DmaLoad16(spec + (size_t(t) * a.height + y) * kTile + (lane % 8) * 2, dst);
    }
  };
  if (blockIdx.x < a.img_h) issue(blockIdx.x);
  for (uint32_t i = threadIdx.x; i < ND1 + kTwdLo; i += TH) tws[i] = twd[i];
  LdsSync();
  InitTwiddles<TH, H, 2, 1, Rs...>(td, ctab, 0, clast, threadIdx.x);
  constexpr uint32_t NP = H / 2 + 1;
  constexpr uint32_t EP = (NP + TH - 1) / TH;
  // the split's twiddles W^-k, W^-(H-k): a thread takes the same bins k in
  // every row, so they are made once (the per-row double products were a
  // tenth of the kernel's VALU)
  Cx<float> wk[EP], wm[EP];
#pragma unroll
  for (uint32_t i = 0; i < EP; ++i) {
    const uint32_t k = threadIdx.x + i * TH;
    if (NP % TH != 0 && k >= NP) continue;
    wk[i] = ToF(TwD(td, k));
    wm[i] = ToF(TwD(td, H - k));
  }
  // fused peak search: this thread's best key over all its rows (value
  // word, then the lowest index), one block reduction at the end: the
  // partials are per workgroup (FastRowsInverseLaunch's n_partials)
  const bool peak = a.peak.partials != nullptr;
  const uint32_t pxs = a.peak.xs, pxn = a.peak.xe - a.peak.xs;
  const uint32_t sign_mask = a.peak.allow_negative != 0 ? 0x7fffffffu : 0xffffffffu;
  uint64_t run_best = 0ull;
  bool first = true;
  for (uint32_t iy = blockIdx.x; iy < a.img_h; iy += gridDim.x) {
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // opaque per row (see Columns)
    // this row's DMA (issued a row ago) landed; the previous row's EH stores
    // per wave, issued after it, may still be in flight
    if (first)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (EH == 16)
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    first = false;
    LdsSync();
    auto zc = [&](Cx<float> xk, Cx<float> xm, Cx<float> w) {
      const Cx<float> sum = {xk.x + xm.x, xk.y - xm.y};
      const Cx<float> dif = {xk.x - xm.x, xk.y + xm.y};
      const Cx<float> t = Mul(Conj(w), dif);
      return Cx<float>{sum.x - t.y, -(sum.y + t.x)};
    };
#pragma unroll
    for (uint32_t i = 0; i < EP; ++i) {
      const uint32_t k = tid + i * TH;
      if (NP % TH != 0 && k >= NP) continue;
      const uint32_t m = H - k;
      Cx<float> xk = raw[k], xm = raw[m];
      if (k == 0) {  // C2R ignores the imaginary parts of X[0] and X[H]
        xk.y = 0.0f;
        xm.y = 0.0f;
      }
      buf[Lx<float>(k)] = zc(xk, xm, wk[i]);
      if (k != 0 && m != k) buf[Lx<float>(m)] = zc(xm, xk, wm[i]);
    }
    LdsSync();  // raw is read: the next row's DMA may overwrite it
    if (iy + gridDim.x < a.img_h) issue(iy + gridDim.x);
    FftC<TH, H, 1, Rs...>(buf, ctab, 0, clast, tid);
    float* o = out + size_t(iy) * a.img_w;
    const bool peak_row = peak && iy >= a.peak.ys && iy < a.peak.ye;
    const uint8_t* mrow = a.peak.mask ? a.peak.mask + size_t(iy) * a.img_w : nullptr;
    // per value the PeakKey value word (|v| or v as bits; 0 when it cannot
    // be a peak: NaN, a negative value without allow_negative, outside the
    // box or the mask); values <= FLT_MIN are excluded by the row's maximum
    uint32_t uq[EH][2];
    uint32_t tb = 0u;
    // the whole plane row is the window (the launcher's condition): every
    // thread stores EH float2, in ascending x
#pragma unroll
    for (uint32_t i = 0; i < EH; ++i) {
      const uint32_t n = tid + i * TH;
      const Cx<float> z = buf[Lx<float>(n)];
      const float2 v = {z.x, -z.y};
      reinterpret_cast<float2*>(o)[n] = v;
      if (peak_row) {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
          const uint32_t x = 2 * n + h;
          const uint32_t u = __float_as_uint(h ? v.y : v.x) & sign_mask;
          const bool q = u <= 0x7f800000u && x - pxs < pxn && (!mrow || mrow[x]);
          uq[i][h] = q ? u : 0u;
          tb = uq[i][h] > tb ? uq[i][h] : tb;
        }
      }
    }
    if (peak_row && tb > 0x00800000u) {
      // the first x holding the row's maximum (x ascends with i, h)
      uint32_t bx = 0u;
#pragma unroll
      for (int i = int(EH) - 1; i >= 0; --i)
#pragma unroll
        for (int h = 1; h >= 0; --h)
          bx = uq[i][h] == tb ? 2 * (tid + uint32_t(i) * TH) + uint32_t(h) : bx;
      const uint64_t key =
          (uint64_t(tb) << 32) | uint64_t(0xffffffffu - (iy * a.img_w + bx));
      run_best = key > run_best ? key : run_best;
    }
    LdsSync();  // the row's LDS reads (buf) before the next row's writes
  }
  if (peak) {
    const uint64_t best = WaveMaxU64(run_best);
    if (lane == 0) red[wave] = best;
    LdsSync();
    if (threadIdx.x < 64) {
      uint64_t w = lane < WAVES ? red[lane] : 0ull;
      w = WaveMaxU64(w);
      if (threadIdx.x == 0) a.peak.partials[blockIdx.x] = w;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// RowsForward (float, whole plane rows -> tiled spectrum) with the next
// image row fetched by LDS-DMA (DmaLoad16: a wave instruction moves 256
// contiguous floats) while this row is transformed and stored, and the pass
// twiddles made once per workgroup (FftC; the register prefetch of the
// persistent kernel left no room for them). The vmcnt count: every wave
// issues at least 2 (EP - 1) >= 16 spectrum stores after the DMA. Same
// arithmetic as RowsForward<float, TH, true>.
template <uint32_t TH, uint32_t... Rs>
__global__ __launch_bounds__(TH) void RowsForwardDma(RowArgs a, const float* __restrict__ in,
                                                     Cx<float>* __restrict__ spec,
                                                     const Cx<double>* __restrict__ twd) {
  constexpr uint32_t H = Product<Rs...>();
  constexpr uint32_t EH = H / TH;
  constexpr uint32_t NP = H / 2 + 1;
  constexpr uint32_t EP = (NP + TH - 1) / TH;
  static_assert(H % TH == 0 && (EH == 16 || EH == 8) && 2 * (EP - 1) >= EH,
                "vmcnt counts of 8 or 16 stores");
  constexpr uint32_t WAVES = TH / 64;
  constexpr uint32_t ND1 = 2 * H / kTwdLo;
  constexpr uint32_t NI = 2 * H / 256;  // DMA wave instructions per row (256 floats each)
  typedef __attribute__((address_space(3))) void* LdsPtr;
  __shared__ __attribute__((aligned(16))) float raw[2 * H];  // the DMA target (see RowsInverseDma)
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<float>* buf = reinterpret_cast<Cx<float>*>(lds_raw);
  Cx<double>* tws = reinterpret_cast<Cx<double>*>(buf + (H + (H >> kFastPadShift)));
  Cx<float>* ctab = reinterpret_cast<Cx<float>*>(tws + ND1 + kTwdLo);
  TwdLds td{tws, tws + ND1};
  Cx<float> clast[LastRadix<Rs...>() - 1];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  auto issue = [&](uint32_t y) {
    const float* row = in + size_t(y) * a.img_w;
    for (uint32_t j = wave; j < NI; j += WAVES) {
      const uint32_t dst = __builtin_amdgcn_readfirstlane(
          uint32_t(uintptr_t((LdsPtr)(raw + j * 256))));
      DmaLoad16(row + j * 256 + lane * 4, dst);
    }
  };
  for (uint32_t i = threadIdx.x; i < ND1 + kTwdLo; i += TH) tws[i] = twd[i];
  if (blockIdx.x < a.height) issue(blockIdx.x);
  LdsSync();
  InitTwiddles<TH, H, 2, 1, Rs...>(td, ctab, 0, clast, threadIdx.x);
  // the split's twiddles W^k, W^(H-k): the same bins in every row of this
  // thread, made once (as RowsInverseDma)
  Cx<float> wk[EP], wm[EP];
#pragma unroll
  for (uint32_t i = 0; i < EP; ++i) {
    const uint32_t k = threadIdx.x + i * TH;
    if (NP % TH != 0 && k >= NP) continue;
    wk[i] = ToF(TwD(td, k));
    wm[i] = ToF(TwD(td, H - k));
  }
  bool first = true;
  for (uint32_t y = blockIdx.x; y < a.height; y += gridDim.x) {
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));  // opaque per row (see Columns)
    if (first)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (EH == 16)
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    first = false;
    LdsSync();
#pragma unroll
    for (uint32_t i = 0; i < EH; ++i) {
      const uint32_t n = tid + i * TH;
      const float2 v = reinterpret_cast<const float2*>(raw)[n];
      buf[Lx<float>(n)] = {v.x, v.y};
    }
    LdsSync();  // raw is read: the next row's DMA may overwrite it
    if (y + gridDim.x < a.height) issue(y + gridDim.x);
    FftC<TH, H, 1, Rs...>(buf, ctab, 0, clast, tid);
    const float h = 0.5f;
    auto put = [&](uint32_t k, Cx<float> zk, Cx<float> zc, Cx<float> w) {
      const Cx<float> ev = {h * (zk.x + zc.x), h * (zk.y + zc.y)};
      const Cx<float> od = {h * (zk.y - zc.y), -h * (zk.x - zc.x)};  // (zk - zc) / 2i
      spec[TileIndex(y, k, a.height)] = Add(ev, Mul(w, od));
    };
#pragma unroll
    for (uint32_t i = 0; i < EP; ++i) {
      const uint32_t k = tid + i * TH;
      if (NP % TH != 0 && k >= NP) continue;
      const Cx<float> zlo = buf[Lx<float>(k)];
      const Cx<float> zhi = k == 0 ? zlo : buf[Lx<float>(H - k)];
      put(k, zlo, Conj(zhi), wk[i]);
      if (H - k != k) put(H - k, zhi, Conj(zlo), wm[i]);
    }
    LdsSync();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace ff

// Supported row lengths (half length H = N / 2), radices in pass order. The
// float plans are here: their kernels take their twiddles from the LDS
// double tables (LT). The double plans (global pass tables) are in
// fft_fast_rows_f64.hip.
#define RDL_FAST_ROWS(T, TH, ...)                                                      \
  FastRows {                                                                           \
    2 * ff::Product<__VA_ARGS__>(), false, TH,                                         \
        reinterpret_cast<const void*>(&ff::RowsInverse<T, TH, true, __VA_ARGS__>),     \
        reinterpret_cast<const void*>(&ff::RowsForward<T, TH, true, __VA_ARGS__>),     \
        MakeRadixList<__VA_ARGS__>(), RowsDma<TH, __VA_ARGS__>(),                      \
        RowsDmaLdsBytes<TH, __VA_ARGS__>(), RowsFwdDma<TH, __VA_ARGS__>(),             \
        RowsFwdDmaLdsBytes<TH, __VA_ARGS__>()                                          \
  }

// the LDS-DMA inverse rows (8 or 16 output pairs per thread) and
// their one dynamic LDS array (RowsInverseDma's layout)
template <uint32_t TH, uint32_t... Rs>
constexpr size_t RowsDmaLdsBytes() {
  constexpr uint32_t H = ff::Product<Rs...>();
  constexpr uint32_t NCT = ff::CachedTableSize<1, Rs...>(TH, H);
  // (the DMA target is a static array of the kernel)
  return size_t(H + (H >> kFastPadShift)) * 8 +
         size_t(2 * H / ff::kTwdLo + ff::kTwdLo) * 16 + size_t(NCT > 0 ? (NCT + 1) / 2 * 2 : 2) * 8 +
         size_t(TH / 64) * 8;
}
template <uint32_t TH, uint32_t... Rs>
constexpr size_t RowsFwdDmaLdsBytes() {
  constexpr uint32_t H = ff::Product<Rs...>();
  constexpr uint32_t NCT = ff::CachedTableSize<1, Rs...>(TH, H);
  return size_t(H + (H >> kFastPadShift)) * 8 + size_t(2 * H / ff::kTwdLo + ff::kTwdLo) * 16 +
         size_t(NCT > 0 ? NCT : 1) * 8;
}
template <uint32_t TH, uint32_t... Rs>
const void* RowsFwdDma() {
  constexpr uint32_t H = ff::Product<Rs...>();
  constexpr uint32_t NP = H / 2 + 1;
  constexpr uint32_t EP = (NP + TH - 1) / TH;
  if constexpr (H % TH == 0 && (H / TH == 16 || H / TH == 8) && 2 * (EP - 1) >= H / TH)
    return reinterpret_cast<const void*>(&ff::RowsForwardDma<TH, Rs...>);
  else
    return nullptr;
}
template <uint32_t TH, uint32_t... Rs>
const void* RowsDma() {
  constexpr uint32_t H = ff::Product<Rs...>();
  if constexpr (H % TH == 0 && (H / TH == 16 || H / TH == 8))
    return reinterpret_cast<const void*>(&ff::RowsInverseDma<TH, Rs...>);
  else
    return nullptr;
}

const FastRows* FindFastRows(uint32_t n, bool f64) {
  static const FastRows kPlans[] = {
      RDL_FAST_ROWS(float, 256, 16, 16, 16),       // 8192
      RDL_FAST_ROWS(float, 256, 16, 16, 8),        // 4096
      RDL_FAST_ROWS(float, 256, 16, 16, 7),        // 3584
      RDL_FAST_ROWS(float, 256, 16, 16, 2, 3),     // 3072
      RDL_FAST_ROWS(float, 256, 16, 16, 5),        // 2560
      RDL_FAST_ROWS(float, 256, 16, 16, 4),        // 2048
      RDL_FAST_ROWS(float, 256, 16, 8, 7),         // 1792
      RDL_FAST_ROWS(float, 256, 16, 16, 3),        // 1536
      RDL_FAST_ROWS(float, 256, 16, 8, 5),         // 1280
  };
  if (f64) return FindFastRowsD(n);
  for (const FastRows& p : kPlans)
    if (p.n == n) return &p;
  return nullptr;
}

#undef RDL_FAST_ROWS

namespace {
// RDL_ROWS_DMA=0: the persistent row kernels where the LDS-DMA ones would run
bool RowsDmaOn() {
  static const bool on = [] {
    const char* e = std::getenv("RDL_ROWS_DMA");
    return !(e && e[0] == '0');
  }();
  return on;
}
// a float plan's kernels read `twd` (MakeTwiddleBase); there is no other path
int NoRowTwiddles() {
  SetError("fast FFT rows: a float plan needs its LDS twiddle base");
  return RDL_ERR_ARG;
}
}  // namespace

int FastRowsInverseLaunch(rdl_session* s, const FastRows* p, const void* spec, float* out,
                          const void* tw, const void* ptw, uint32_t height, uint32_t img_w, uint32_t img_h,
                          uint32_t ox, uint32_t oy, int subtract, int tiled, const RowPeak* peak,
                          const void* twd, uint32_t* n_partials) {
  // the LDS-DMA kernel: a tiled float spectrum written whole into the
  // window (RDL_ROWS_DMA=0: the persistent row kernel)
  if (n_partials) *n_partials = img_h;  // per-row partials (the persistent row kernel)
  const uint32_t half = p->n / 2;
  if (RowsDmaOn() && p->inverse_dma && twd && tiled && !subtract && ox == 0 && img_w == p->n &&
      img_h > 0) {
    const size_t lds = p->inverse_dma_lds;
    const int slots = SlotsPerCu(s, p->inverse_dma, p->threads, lds);
    if (slots < 0) {
      SetError("fast FFT rows (DMA): occupancy query failed");
      return RDL_ERR_HIP;
    }
    ff::RowArgs a{};
    a.height = height;
    a.ld = half + 1;
    a.img_w = img_w;
    a.img_h = img_h;
    a.ox = ox;
    a.oy = oy;
    a.tiled = 1;
    if (peak) a.peak = *peak;
    const uint32_t grid = std::min<uint32_t>(img_h, uint32_t(s->n_cus) * uint32_t(slots));
    void* args[] = {&a, (void*)&spec, (void*)&out, (void*)&twd};
    RDL_HIP_CHECK(hipLaunchKernel(p->inverse_dma, dim3(grid), dim3(p->threads), args, lds,
                                  s->stream));
    if (n_partials) *n_partials = grid;  // one partial per workgroup
    return RDL_OK;
  }
  const size_t lds = FastLdsBytes(p->n / 2, p->f64);
  if (!p->f64 && !twd) return NoRowTwiddles();
  const void* fn = p->inverse;
  const int slots = SlotsPerCu(s, fn, p->threads, lds);
  if (slots < 0) {
    SetError("fast FFT rows: occupancy query failed");
    return RDL_ERR_HIP;
  }
  if (img_h == 0) return RDL_OK;
  ff::RowArgs a{};
  a.height = height;
  a.ld = p->n / 2 + 1;
  a.img_w = img_w;
  a.img_h = img_h;
  a.ox = ox;
  a.oy = oy;
  a.subtract = subtract;
  a.tiled = tiled;
  if (peak) a.peak = *peak;
  // RDL_ROWS_RPRE=0: the residual read where it is subtracted (comparison)
  static const int rpre = [] {
    const char* e = std::getenv("RDL_ROWS_RPRE");
    return (e && e[0] == '0') ? 0 : 1;
  }();
  a.prefetch = rpre;
  // The float (LT) kernels are persistent (rows grid-strided): one table load per workgroup.
  // A session with a second lane keeps one slot per CU free for the other
  // lane's column passes (8192^2 bench: 762.8 -> 757.3 ms per step; 770.9
  // with one lane), RDL_ROWS_PER_CU sets the cap
  static const int cap_env = [] {
    const char* e = std::getenv("RDL_ROWS_PER_CU");
    return e ? std::atoi(e) : 0;
  }();
  const int cap = cap_env > 0 ? cap_env : (s->aux && slots >= 4 ? slots - 1 : slots);
  const uint32_t per_cu = uint32_t(cap < slots ? cap : slots);
  const uint32_t grid =
      !p->f64 ? std::min<uint32_t>(img_h, uint32_t(s->n_cus) * per_cu) : img_h;
  void* args[] = {&a, (void*)&spec, (void*)&out, (void*)&tw, (void*)&ptw, (void*)&twd};
  RDL_HIP_CHECK(hipLaunchKernel(fn, dim3(grid), dim3(p->threads), args, lds, s->stream));
  return RDL_OK;
}

int FastRowsForwardLaunch(rdl_session* s, const FastRows* p, const float* in, void* spec,
                          const void* tw, const void* ptw, uint32_t height, uint32_t img_w, uint32_t img_h,
                          uint32_t ox, uint32_t oy, const uint32_t* rows,
                          const uint32_t* n_rows, int tiled, const void* twd, int all_rows) {
  // the LDS-DMA kernel: a whole float plane into a tiled spectrum
  // (RDL_ROWS_DMA=0: the persistent row kernel)
  if (RowsDmaOn() && p->forward_dma && twd && tiled && !rows && ox == 0 &&
      oy == 0 && img_w == p->n && img_h == height && height > 0) {
    const size_t lds = p->forward_dma_lds;
    const int slots = SlotsPerCu(s, p->forward_dma, p->threads, lds);
    if (slots < 0) {
      SetError("fast FFT rows (DMA): occupancy query failed");
      return RDL_ERR_HIP;
    }
    ff::RowArgs a{};
    a.height = height;
    a.ld = p->n / 2 + 1;
    a.img_w = img_w;
    a.img_h = img_h;
    a.tiled = 1;
    a.all_rows = 1;
    const uint32_t grid = std::min<uint32_t>(height, uint32_t(s->n_cus) * uint32_t(slots));
    void* args[] = {&a, (void*)&in, (void*)&spec, (void*)&twd};
    RDL_HIP_CHECK(hipLaunchKernel(p->forward_dma, dim3(grid), dim3(p->threads), args, lds,
                                  s->stream));
    return RDL_OK;
  }
  const size_t lds = FastLdsBytes(p->n / 2, p->f64);
  if (!p->f64 && !twd) return NoRowTwiddles();
  const void* fn = p->forward;
  const int slots = SlotsPerCu(s, fn, p->threads, lds);
  if (slots < 0) {
    SetError("fast FFT rows: occupancy query failed");
    return RDL_ERR_HIP;
  }
  ff::RowArgs a{};
  a.height = height;
  a.ld = p->n / 2 + 1;
  a.img_w = img_w;
  a.img_h = img_h;
  a.ox = ox;
  a.oy = oy;
  a.rows = rows;
  a.n_rows = n_rows;
  a.tiled = tiled;
  // (all_rows < 0: every plane row for a tiled spectrum, the window rows otherwise)
  a.all_rows = all_rows < 0 ? tiled : all_rows;
  const uint32_t max_rows = (rows || a.all_rows) ? height : img_h;
  if (max_rows == 0) return RDL_OK;
  const uint32_t grid =
      std::min<uint32_t>(max_rows, uint32_t(s->n_cus) * uint32_t(slots) * 2);
  void* args[] = {&a, (void*)&in, (void*)&spec, (void*)&tw, (void*)&ptw, (void*)&twd};
  RDL_HIP_CHECK(hipLaunchKernel(fn, dim3(grid), dim3(p->threads), args, lds, s->stream));
  return RDL_OK;
}

}  // namespace rdl
