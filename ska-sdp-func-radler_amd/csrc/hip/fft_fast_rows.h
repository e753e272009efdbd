// The row kernels that both precisions instantiate (RowsInverse,
// RowsForward), for the two units that hold their plan tables:
// fft_fast_rows.hip (float, the LDS-DMA kernels, the launchers) and
// fft_fast_rows_f64.hip (double).
#pragma once

#include <type_traits>

#include "fft_fast_internal.h"

namespace rdl {
namespace ff {

// ----------------------------------------------------------------- rows
// One real row of length 2H per workgroup, as a half-length complex FFT
// (z[n] = x[2n] + i x[2n+1]) with the even/odd split folded in: H complex in
// LDS (72 KiB for H = 4536 double), so two workgroups share a CU and one's
// loads overlap the other's transform. Twiddles: the length-2H table.
struct RowArgs {
  uint32_t height;      // plane rows
  uint32_t ld;          // spectrum row stride (H + 1)
  uint32_t img_w, img_h, ox, oy;  // image window inside the plane
  const uint32_t* rows;    // forward: the non-zero plane rows (NULL: the window rows)
  const uint32_t* n_rows;  // their count (device)
  int subtract;         // inverse: 0 write, 1 subtract from out
  int tiled;            // spectrum in column tiles (see TileIndex), else row-major
  int all_rows;         // forward: every plane row (zero outside the window)
  RowPeak peak;         // inverse: fused peak search when peak.partials
  int prefetch;         // inverse, subtract: load the residual row before the transform
};


// spectrum rows (X[0..H]) -> real rows written into / subtracted from the
// window. Z[k] = (X[k] + conj X[H-k]) + i W^-k (X[k] - conj X[H-k]) gives
// z = IFFT_H(Z) = N (x_even + i x_odd) (unnormalised, as C2R); the inverse
// runs as conj(FFT(conj Z)). The imaginary parts of X[0] and X[H] are
// ignored, as by C2R.
// LT (float only): twiddles from the LDS double tables (TwdLds, `twd` = the
// base table of length 2H: 2H / 64 entries W^{64 i}, then 64 entries W^i)
// and persistent workgroups (rows blockIdx, blockIdx + grid, ...: the table
// is loaded once per workgroup).
template <typename T, uint32_t TH, bool LT, uint32_t... Rs>
__global__ __launch_bounds__(TH) void RowsInverse(RowArgs a, const Cx<T>* __restrict__ spec,
                                                  float* __restrict__ out,
                                                  const Cx<T>* __restrict__ tw,
                                                  const Cx<T>* __restrict__ ptw,
                                                  const Cx<double>* __restrict__ twd) {
  constexpr uint32_t H = Product<Rs...>();
  constexpr uint32_t EH = (H + TH - 1) / TH;
  constexpr uint32_t ND1 = LT ? 2 * H / kTwdLo : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  __shared__ uint64_t red[TH / 64];  // fused peak search
  __shared__ Cx<double> tws[LT ? ND1 + kTwdLo : 1];
  TwdLds td{tws, tws + ND1};
  // LT: the pass twiddles, made once per workgroup (FftC)
  constexpr uint32_t NCT = LT ? CachedTableSize<1, Rs...>(TH, H) : 0;
  __shared__ Cx<float> ctab[NCT > 0 ? NCT : 1];
  Cx<float> clast[LT ? LastRadix<Rs...>() - 1 : 1];
  if constexpr (LT) {
    for (uint32_t i = threadIdx.x; i < ND1 + kTwdLo; i += TH) tws[i] = twd[i];
    __syncthreads();
    InitTwiddles<TH, H, 2, 1, Rs...>(td, ctab, 0, clast, threadIdx.x);
    __syncthreads();
  }
  // bins in pairs (k, H - k): every spectrum element is read once
  constexpr uint32_t NP = H / 2 + 1;
  constexpr uint32_t EP = (NP + TH - 1) / TH;
  auto row_ptr = [&](uint32_t iy) { return spec + size_t(iy + a.oy) * a.ld; };
  auto load_at = [&](uint32_t iy, uint32_t k) {
    return *(a.tiled ? spec + TileIndex(iy + a.oy, k, a.height) : row_ptr(iy) + k);
  };
  // (the next row's bins prefetched into registers measured slower: 186.6 ->
  // 205.8 us per 8192^2 pass on MI355X, the registers cost a wave per SIMD)
  for (uint32_t iy = blockIdx.x; iy < a.img_h; iy += LT ? gridDim.x : a.img_h) {
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque per row (see Columns)
  // conj(Z) for bin k from X[k] = xk and X[H-k] = xm
  auto zc = [&](Cx<T> xk, Cx<T> xm, uint32_t k) {
    const Cx<T> sum = {xk.x + xm.x, xk.y - xm.y};  // X[k] + conj X[H-k]
    const Cx<T> dif = {xk.x - xm.x, xk.y + xm.y};  // X[k] - conj X[H-k]
    Cx<T> wk;
    if constexpr (LT)
      wk = ToF(TwD(td, k));
    else
      wk = tw[k];
    const Cx<T> t = Mul(Conj(wk), dif);           // W_N^-k (...)
    return Cx<T>{sum.x - t.y, -(sum.y + t.x)};      // Z = sum + i t, conjugated
  };
#pragma unroll
  for (uint32_t i = 0; i < EP; ++i) {
    const uint32_t k = tid + i * TH;
    if (NP % TH != 0 && k >= NP) continue;
    const uint32_t m = H - k;
    Cx<T> xk = load_at(iy, k), xm = load_at(iy, m);
    if (k == 0) {  // C2R ignores the imaginary parts of X[0] and X[H]
      xk.y = T(0);
      xm.y = T(0);
    }
    buf[Lx<T>(k)] = zc(xk, xm, k);
    if (k != 0 && m != k) buf[Lx<T>(m)] = zc(xm, xk, m);
  }
  float* o = out + size_t(iy) * a.img_w;
  // subtract (the residual correction): the row's residual values loaded
  // now, issued after the spectrum loads, so they arrive during the
  // transform instead of after it (LdsSync waits for LDS only)
  const bool even_win = ((a.ox | a.img_w) & 1u) == 0;
  // only the 512-thread float64 plans (the 8192^2 / 4096^2 corrections'):
  // the registers cost the smaller plans a wave per SIMD (the gridded runs'
  // subimage corrections: 7 -> 5 waves at 128 threads, measured slower)
  constexpr bool kRpre = std::is_same_v<T, double> && TH >= 512;
  float2 rpre[kRpre ? EH : 1];
  if (kRpre && a.subtract && a.prefetch && even_win) {
#pragma unroll
    for (uint32_t i = 0; i < EH; ++i) {
      const uint32_t n = tid + i * TH;
      if (H % TH != 0 && n >= H) continue;
      const uint32_t x0 = 2 * n;
      if (x0 < a.ox || x0 >= a.ox + a.img_w) continue;
      rpre[i] = *reinterpret_cast<const float2*>(o + (x0 - a.ox));
    }
  }
  LdsSync();
  if constexpr (LT)
    FftC<TH, H, 1, Rs...>(buf, ctab, 0, clast, tid);
  else
    Fft<T, TH, H, 0, 1, Rs...>(buf, ptw, tid);
  // fused peak search over the values as written (window coordinates): per
  // thread the largest PeakKey value word (0: none qualifies) and its first
  // x, in 32-bit compares (a thread visits its x in ascending order, so the
  // strict > keeps the first of equal values, as PeakKey's index word does);
  // one 64-bit key per thread at the end of the row
  const bool peak = a.peak.partials != nullptr;
  const bool peak_row = peak && iy >= a.peak.ys && iy < a.peak.ye;
  const uint32_t pxs = a.peak.xs, pxn = a.peak.xe - a.peak.xs;
  const uint8_t* mrow = a.peak.mask ? a.peak.mask + size_t(iy) * a.img_w : nullptr;
  const uint32_t sign_mask = a.peak.allow_negative != 0 ? 0x7fffffffu : 0xffffffffu;
  uint32_t best_u = 0u, best_x = 0u;
  auto consider = [&](uint32_t x, float v) {
    if (!peak_row) return;
    const uint32_t u = __float_as_uint(v) & sign_mask;
    const bool q = u > 0x00800000u && u <= 0x7f800000u && x - pxs < pxn &&
                   (!mrow || mrow[x]);
    const uint32_t uq = q ? u : 0u;
    const bool better = uq > best_u;
    best_u = better ? uq : best_u;
    best_x = better ? x : best_x;
  };
  auto finish_peak = [&]() {
    if (!peak) return;
    uint64_t best = best_u ? ((uint64_t(best_u) << 32) |
                              uint64_t(0xffffffffu - (iy * a.img_w + best_x)))
                           : 0ull;
    best = BlockMaxU64(best, red);
    if (tid == 0) a.peak.partials[iy] = best;
  };
  if (even_win) {
    // even window: (x[2n], x[2n+1]) both in or both out, one 8-B access
#pragma unroll
    for (uint32_t i = 0; i < EH; ++i) {
      const uint32_t n = tid + i * TH;
      if (H % TH != 0 && n >= H) continue;
      const uint32_t x0 = 2 * n;
      if (x0 < a.ox || x0 >= a.ox + a.img_w) continue;
      const Cx<T> z = buf[Lx<T>(n)];  // conj(result): x[2n] = z.x, x[2n+1] = -z.y
      float2* p = reinterpret_cast<float2*>(o + (x0 - a.ox));
      float2 v = {float(z.x), float(-z.y)};
      if (a.subtract) {
        const float2 r = (kRpre && a.prefetch) ? rpre[kRpre ? i : 0] : *p;
        v = {r.x - v.x, r.y - v.y};
      }
      *p = v;
      consider(x0 - a.ox, v.x);
      consider(x0 - a.ox + 1, v.y);
    }
    finish_peak();
    if constexpr (LT) LdsSync();  // the row's LDS reads before the next row's stores
    continue;
  }
#pragma unroll
  for (uint32_t i = 0; i < EH; ++i) {
    const uint32_t n = tid + i * TH;
    if (H % TH != 0 && n >= H) continue;
    const Cx<T> z = buf[Lx<T>(n)];
    const uint32_t x0 = 2 * n, x1 = x0 + 1;
    if (x0 >= a.ox && x0 < a.ox + a.img_w) {
      float* p = o + (x0 - a.ox);
      const float v = a.subtract ? *p - float(z.x) : float(z.x);
      *p = v;
      consider(x0 - a.ox, v);
    }
    if (x1 >= a.ox && x1 < a.ox + a.img_w) {
      float* p = o + (x1 - a.ox);
      const float v = a.subtract ? *p - float(-z.y) : float(-z.y);
      *p = v;
      consider(x1 - a.ox, v);
    }
  }
  finish_peak();
  if constexpr (LT) LdsSync();
  }
}

// real plane rows (the window's image rows, zero outside) -> spectrum rows
// X[0..H]: X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[H-k]) / 2,
// O = (Z[k] - conj Z[H-k]) / 2i. Rows not listed are not touched (the
// column pass reads only listed rows).
template <typename T, uint32_t TH, bool LT, uint32_t... Rs>
__global__ __launch_bounds__(TH) void RowsForward(RowArgs a, const float* __restrict__ in,
                                                  Cx<T>* __restrict__ spec,
                                                  const Cx<T>* __restrict__ tw,
                                                  const Cx<T>* __restrict__ ptw,
                                                  const Cx<double>* __restrict__ twd) {
  constexpr uint32_t H = Product<Rs...>();
  constexpr uint32_t EH = (H + TH - 1) / TH;
  constexpr uint32_t ND1 = LT ? 2 * H / kTwdLo : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  __shared__ Cx<double> tws[LT ? ND1 + kTwdLo : 1];
  TwdLds td{tws, tws + ND1};
  // (the per-row twiddle math stays: with the next row's input prefetched in
  // registers, FftC's cached last-pass twiddles would cost a wave per SIMD)
  if constexpr (LT) {
    for (uint32_t i = threadIdx.x; i < ND1 + kTwdLo; i += TH) tws[i] = twd[i];
    __syncthreads();
  }
  const uint32_t n_rows = a.rows ? *a.n_rows : (a.all_rows ? a.height : a.img_h);
  const bool even = ((a.ox | a.img_w) & 1u) == 0;
  auto row_of = [&](uint32_t r) { return a.rows ? a.rows[r] : (a.all_rows ? r : r + a.oy); };
  // (e, o) = (x[2n], x[2n+1]) of plane row y, zero outside the window
  auto pair_at = [&](uint32_t y, uint32_t n) {
    const int64_t iy = int64_t(y) - a.oy;
    const bool in_y = iy >= 0 && iy < a.img_h;
    const float* row = in + (in_y ? size_t(iy) * a.img_w : 0);
    const uint32_t x0 = 2 * n, x1 = x0 + 1;
    float2 v = {0.0f, 0.0f};
    if (even) {  // (x[2n], x[2n+1]) both in or both out: one 8-B load
      if (in_y && x0 >= a.ox && x0 < a.ox + a.img_w)
        v = *reinterpret_cast<const float2*>(row + (x0 - a.ox));
    } else {
      v.x = in_y && x0 >= a.ox && x0 < a.ox + a.img_w ? row[x0 - a.ox] : 0.0f;
      v.y = in_y && x1 >= a.ox && x1 < a.ox + a.img_w ? row[x1 - a.ox] : 0.0f;
    }
    return v;
  };
  // LT: the next row's input is loaded into registers before this row's
  // transform and stores (see RowsInverse)
  float2 pre[EH];
  auto prefetch = [&](uint32_t r, uint32_t tid) {
    const uint32_t y = row_of(r);
#pragma unroll
    for (uint32_t i = 0; i < EH; ++i) {
      const uint32_t n = tid + i * TH;
      if (H % TH != 0 && n >= H) continue;
      pre[i] = pair_at(y, n);
    }
  };
  if constexpr (LT)
    if (blockIdx.x < n_rows) prefetch(blockIdx.x, threadIdx.x);
  for (uint32_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    uint32_t tid = threadIdx.x;  // opaque per row (see Columns)
    asm volatile("" : "+v"(tid));
    const uint32_t y = row_of(r);
#pragma unroll
    for (uint32_t i = 0; i < EH; ++i) {
      const uint32_t n = tid + i * TH;
      if (H % TH != 0 && n >= H) continue;
      float2 v;
      if constexpr (LT)
        v = pre[i];
      else
        v = pair_at(y, n);
      buf[Lx<T>(n)] = {T(v.x), T(v.y)};
    }
    if constexpr (LT)
      if (r + gridDim.x < n_rows) prefetch(r + gridDim.x, tid);
    LdsSync();
    if constexpr (LT)
      FftL<TH, H, 2, 1, Rs...>(buf, td, tid);
    else
      Fft<T, TH, H, 0, 1, Rs...>(buf, ptw, tid);
    Cx<T>* X = spec + size_t(y) * a.ld;
    const T h = T(0.5);
    // X[k] from (Z[k], conj Z[H-k]) and X[H-k] from (Z[H-k], conj Z[k]): the
    // bins in pairs, each LDS value read once (X[0] and X[H] both come from
    // Z[0]); every output is the same expression as bin by bin
    auto put = [&](uint32_t k, Cx<T> zk, Cx<T> zc) {
      const Cx<T> ev = {h * (zk.x + zc.x), h * (zk.y + zc.y)};
      const Cx<T> od = {h * (zk.y - zc.y), -h * (zk.x - zc.x)};  // (zk - zc) / 2i
      Cx<T> wk;
      if constexpr (LT)
        wk = ToF(TwD(td, k));
      else
        wk = tw[k];
      const Cx<T> v = Add(ev, Mul(wk, od));
      // one address, one 8/16-byte store (a store per layout branch was
      // split into scalar halves)
      *(a.tiled ? spec + TileIndex(y, k, a.height) : X + k) = v;
    };
    constexpr uint32_t NP = H / 2 + 1;
    constexpr uint32_t EP = (NP + TH - 1) / TH;
#pragma unroll
    for (uint32_t i = 0; i < EP; ++i) {
      const uint32_t k = tid + i * TH;
      if (NP % TH != 0 && k >= NP) continue;
      const Cx<T> zlo = buf[Lx<T>(k)];
      const Cx<T> zhi = k == 0 ? zlo : buf[Lx<T>(H - k)];
      put(k, zlo, Conj(zhi));
      if (H - k != k) put(H - k, zhi, Conj(zlo));
    }
    LdsSync();
  }
}

}  // namespace ff

/* the float64 plan of row length n, or nullptr (fft_fast_rows_f64.hip) */
const FastRows* FindFastRowsD(uint32_t n);

}  // namespace rdl
