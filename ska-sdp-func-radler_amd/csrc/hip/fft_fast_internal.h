// What the fft_fast_*.hip units share: the device helpers of the
// compile-time-planned transforms (passes, twiddle tables, layouts) and the
// launchers' occupancy query. Each kernel family, with its plan table and
// launch function, lives in one unit: fft_fast_cols.hip (Columns),
// fft_fast_convd.hip (ColumnsConvD), fft_fast_rows.hip (the row kernels),
// fft_fast_steps.hip (the four-step passes); fft_fast.hip holds the tables
// made on the host. conv.hip sees fft_fast.h only.
#pragma once

#include <cstddef>
#include <cstdint>

#include "fft_dft.h"
#include "fft_fast.h"
#include "rdl_internal.h"

namespace rdl {
namespace ff {

// Orders LDS only: __syncthreads() would also drain the prefetch loads.
__device__ __forceinline__ void LdsSync() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// LDS slot of logical element i of a transform (see kFastPadShift)
template <typename T>
__device__ __forceinline__ uint32_t Lx(uint32_t i) {
  if constexpr (sizeof(T) == 4)
    return i + (i >> kFastPadShift);
  else
    return i;
}

// One Stockham pass (radix R, span NS) over a length-N transform in LDS, in
// place (inputs read to registers before the barrier). Twiddles come from the
// plan's pass table (MakePassTable, host): pass p's W_N^{k (q+1) M} at
// ptw[OFF + q NS + k], so a wave's load for one q is one contiguous run.
// Float reads every power; double reads w and builds w^r by recurrence (error
// ~1e-15, far below the float rounding of the result).
template <typename T, uint32_t TH, uint32_t N, uint32_t R, uint32_t NS, uint32_t OFF>
__device__ __forceinline__ void Pass(Cx<T>* buf, const Cx<T>* __restrict__ ptw,
                                     uint32_t tid) {
  constexpr uint32_t NB = N / R;
  constexpr uint32_t BPT = (NB + TH - 1) / TH;
  constexpr bool kTable = sizeof(T) == 4;
  constexpr uint32_t NW = NS > 1 ? (kTable ? R - 1 : 1) : 1;
  Cx<T> v[BPT][R];
  Cx<T> w[BPT][NW];
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
      if constexpr (NS > 1) {
        const uint32_t k = j % NS;
#pragma unroll
        for (uint32_t q = 0; q < NW; ++q) w[i][q] = ptw[OFF + q * NS + k];
      }
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) v[i][r] = buf[Lx<T>(j + r * NB)];
    }
  }
  LdsSync();
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
      const uint32_t k = j % NS;
      if constexpr (NS > 1) {
        if constexpr (kTable) {
#pragma unroll
          for (uint32_t r = 1; r < R; ++r) v[i][r] = Mul(v[i][r], w[i][r - 1]);
        } else {
          Cx<T> wr = w[i][0];
          v[i][1] = Mul(v[i][1], wr);
#pragma unroll
          for (uint32_t r = 2; r < R; ++r) {
            wr = Mul(wr, w[i][0]);
            v[i][r] = Mul(v[i][r], wr);
          }
        }
      }
      Dft<T, int(R)>::Run(v[i]);
      const uint32_t d = (j / NS) * NS * R + k;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) buf[Lx<T>(d + r * NS)] = v[i][r];
    }
  }
  LdsSync();
}

// entries of pass (radix R, span NS) in the pass table
constexpr uint32_t PassTableSize(uint32_t R, uint32_t NS) { return NS > 1 ? NS * (R - 1) : 0; }

template <typename T, uint32_t TH, uint32_t N, uint32_t OFF, uint32_t NS, uint32_t R,
          uint32_t... Rest>
__device__ __forceinline__ void Fft(Cx<T>* buf, const Cx<T>* __restrict__ ptw,
                                    uint32_t tid) {
  Pass<T, TH, N, R, NS, OFF>(buf, ptw, tid);
  if constexpr (sizeof...(Rest) > 0)
    Fft<T, TH, N, OFF + PassTableSize(R, NS), NS * R, Rest...>(buf, ptw, tid);
}

template <uint32_t... Rs>
constexpr uint32_t Product() {
  return (Rs * ... * 1u);
}

// Float transforms with their twiddles computed from two small double tables
// in LDS instead of loaded per butterfly from the global pass tables (which
// made three quarters of the row kernels' load instructions, PMC
// SQ_INSTS_VMEM_RD): W_L^e = D1[e >> 6] x D2[e & 63] in double (exact table
// entries), powers by recurrence in double, each rounded to float once —
// the float pass table's values (long double, rounded) but for the rare
// rounding tie. L = SC x N (the base length, rows: 2H).
constexpr uint32_t kTwdLo = 64;
struct TwdLds {
  const Cx<double>* d1;  // W_L^{64 i}
  const Cx<double>* d2;  // W_L^i, i < 64
};
__device__ __forceinline__ Cx<double> TwD(const TwdLds& t, uint32_t e) {
  return Mul(t.d1[e / kTwdLo], t.d2[e % kTwdLo]);
}
__device__ __forceinline__ Cx<float> ToF(Cx<double> v) { return {float(v.x), float(v.y)}; }

template <uint32_t TH, uint32_t N, uint32_t R, uint32_t NS, uint32_t SC>
__device__ __forceinline__ void PassL(Cx<float>* buf, const TwdLds& td, uint32_t tid) {
  constexpr uint32_t NB = N / R;
  constexpr uint32_t BPT = (NB + TH - 1) / TH;
  Cx<float> v[BPT][R];
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) v[i][r] = buf[Lx<float>(j + r * NB)];
    }
  }
  LdsSync();
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
      const uint32_t k = j % NS;
      if constexpr (NS > 1) {
        const Cx<double> w = TwD(td, k * (N / (NS * R)) * SC);
        Cx<double> wr = w;
        v[i][1] = Mul(v[i][1], ToF(wr));
#pragma unroll
        for (uint32_t r = 2; r < R; ++r) {
          wr = Mul(wr, w);
          v[i][r] = Mul(v[i][r], ToF(wr));
        }
      }
      Dft<float, int(R)>::Run(v[i]);
      const uint32_t d = (j / NS) * NS * R + k;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) buf[Lx<float>(d + r * NS)] = v[i][r];
    }
  }
  LdsSync();
}

template <uint32_t TH, uint32_t N, uint32_t SC, uint32_t NS, uint32_t R, uint32_t... Rest>
__device__ __forceinline__ void FftL(Cx<float>* buf, const TwdLds& td, uint32_t tid) {
  PassL<TH, N, R, NS, SC>(buf, td, tid);
  if constexpr (sizeof...(Rest) > 0) FftL<TH, N, SC, NS * R, Rest...>(buf, td, tid);
}

// The same transform with its pass twiddles computed ONCE per workgroup (the
// persistent row kernels transform many rows, and a thread's butterflies
// are the same in every row): PassL's float values (double recurrence, each
// power rounded once), kept in registers for a last pass with one butterfly
// per thread and in a small LDS table [q NS + k] for every other pass with
// twiddles. Same values, same arithmetic: bit-identical to FftL, without
// its per-row double math (the row kernels' largest VALU cost).
template <uint32_t NS, uint32_t R, uint32_t... Rest>
constexpr uint32_t CachedTableSize(uint32_t th, uint32_t n) {
  // entries of the LDS tables: every pass with NS > 1 except a last pass
  // with one butterfly per thread (registers)
  const bool last = sizeof...(Rest) == 0;
  const bool regs = last && (n / R + th - 1) / th == 1;
  const uint32_t here = (NS > 1 && !regs) ? NS * (R - 1) : 0;
  if constexpr (sizeof...(Rest) > 0)
    return here + CachedTableSize<NS * R, Rest...>(th, n);
  else
    return here;
}

template <uint32_t... Rs>
constexpr uint32_t LastRadix() {
  constexpr uint32_t r[] = {Rs...};
  return r[sizeof...(Rs) - 1];
}

template <uint32_t TH, uint32_t N, uint32_t SC, uint32_t NS, uint32_t R, uint32_t... Rest>
__device__ __forceinline__ void InitTwiddles(const TwdLds& td, Cx<float>* table, uint32_t off,
                                             Cx<float>* last, uint32_t tid) {
  constexpr uint32_t NB = N / R;
  constexpr bool kLast = sizeof...(Rest) == 0;
  constexpr bool kRegs = kLast && (NB + TH - 1) / TH == 1;
  if constexpr (NS > 1) {
    if constexpr (kRegs) {
      const uint32_t k = tid % NS;
      const Cx<double> w = TwD(td, k * (N / (NS * R)) * SC);
      Cx<double> wr = w;
      last[0] = ToF(wr);
#pragma unroll
      for (uint32_t r = 2; r < R; ++r) {
        wr = Mul(wr, w);
        last[r - 1] = ToF(wr);
      }
    } else {
      for (uint32_t k = tid; k < NS; k += TH) {
        const Cx<double> w = TwD(td, k * (N / (NS * R)) * SC);
        Cx<double> wr = w;
        table[off + k] = ToF(wr);
        for (uint32_t r = 2; r < R; ++r) {
          wr = Mul(wr, w);
          table[off + (r - 1) * NS + k] = ToF(wr);
        }
      }
    }
  }
  if constexpr (!kLast)
    InitTwiddles<TH, N, SC, NS * R, Rest...>(td, table,
                                             off + ((NS > 1 && !kRegs) ? NS * (R - 1) : 0), last,
                                             tid);
}

template <uint32_t TH, uint32_t N, uint32_t R, uint32_t NS, bool kLast>
__device__ __forceinline__ void PassC(Cx<float>* buf, const Cx<float>* table, uint32_t off,
                                      const Cx<float>* last, uint32_t tid) {
  constexpr uint32_t NB = N / R;
  constexpr uint32_t BPT = (NB + TH - 1) / TH;
  constexpr bool kRegs = kLast && BPT == 1;
  Cx<float> v[BPT][R];
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) v[i][r] = buf[Lx<float>(j + r * NB)];
    }
  }
  LdsSync();
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
      const uint32_t k = j % NS;
      if constexpr (NS > 1) {
#pragma unroll
        for (uint32_t r = 1; r < R; ++r)
          v[i][r] = Mul(v[i][r], kRegs ? last[r - 1] : table[off + (r - 1) * NS + k]);
      }
      Dft<float, int(R)>::Run(v[i]);
      const uint32_t d = (j / NS) * NS * R + k;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) buf[Lx<float>(d + r * NS)] = v[i][r];
    }
  }
  LdsSync();
}

template <uint32_t TH, uint32_t N, uint32_t NS, uint32_t R, uint32_t... Rest>
__device__ __forceinline__ void FftC(Cx<float>* buf, const Cx<float>* table, uint32_t off,
                                     const Cx<float>* last, uint32_t tid) {
  constexpr bool kLast = sizeof...(Rest) == 0;
  constexpr bool kRegs = kLast && (N / R + TH - 1) / TH == 1;
  PassC<TH, N, R, NS, kLast>(buf, table, off, last, tid);
  if constexpr (!kLast)
    FftC<TH, N, NS * R, Rest...>(buf, table, off + ((NS > 1 && !kRegs) ? NS * (R - 1) : 0),
                                 last, tid);
}

// arguments of the column kernels (Columns, ColumnsConvD)
struct ColArgs {
  uint32_t n_cols;    // spectrum columns = width / 2 + 1
  uint32_t ld;        // row stride of row-major buffers (= n_cols)
  uint32_t mode;      // 0 forward; 1 forward, x K x s, inverse; 2 x K x s, inverse
  uint32_t in_cm, out_cm, kern_cm;  // column-major layouts (column c at c * N)
  const uint32_t* rows;    // modes 0/1: the input's non-zero rows, or NULL:
  const uint32_t* n_rows;  //   rows [row0, row0 + row_n) (their count: device)
  uint32_t row0, row_n;
  uint32_t per_xcd;   // columns each XCD takes per round (grid / 8)
  double scale;
  // ColumnsConvD: output rows outside [out_row0, out_row0 + out_row_n) are
  // not written (the inverse row pass reads the output window's rows only)
  uint32_t out_row0, out_row_n;
  // ColumnsConvD: input and output in the tiled layout (TileIndex, column
  // length N) instead of row-major
  uint32_t tiled;
};

// Tiled spectrum layout of the four-step column passes: 16 adjacent columns
// (128 B of float complex, 256 B of double complex) of every row side by side, tile after tile, so
// both the row passes and the column passes move whole cache lines.
constexpr uint32_t kTile = 16;
__device__ __forceinline__ size_t TileIndex(uint32_t y, uint32_t k, uint32_t height) {
  return (size_t(k / kTile) * height + y) * kTile + (k % kTile);
}

}  // namespace ff

// workgroups per CU for a kernel at its LDS size (cached), after raising its
// dynamic LDS limit once per device; < 0: a HIP query failed (fft_fast.hip)
int SlotsPerCu(rdl_session* s, const void* fn, uint32_t threads, size_t lds);

}  // namespace rdl
