// The float64 correction columns of the compile-time-planned FFT engine (see
// fft_fast.hip), their plans and launcher.
#include <algorithm>
#include <type_traits>

#include "fft_fast_internal.h"

namespace rdl {
namespace ff {

// ----------------------------------- float64 correction columns (mode 1)
// ColumnsConvD: the column pass of CorrectResidualDirty's padded convolution
// (forward, x K x s, inverse; sparse input rows; input and output row-major
// or, ColArgs::tiled, in the tiled layout), with the
// per-round latency chain of Columns cut down:
//   * pass twiddles from two small LDS tables (W^e = T1[e >> 7] T2[e & 127],
//     both exact entries of the plan's length-N table) instead of a global
//     load per butterfly and pass,
//   * the first forward pass reads the input straight from global memory
//     through a row bitmap in LDS (no staging, no zeroing sweep per column),
//   * the last forward pass multiplies by K x s (prefetched into registers in
//     that pass's output order) and conjugates before its LDS store (no
//     separate multiply sweep),
//   * the last inverse pass stores to global memory from its registers.
// Same arithmetic as Columns up to the twiddle products' last bit (results
// are rounded to float by the row pass; tests/test_fft_fast.py).
constexpr uint32_t kTwShift = 7;
constexpr uint32_t kTwLo = 1u << kTwShift;

template <uint32_t TH, uint32_t N, uint32_t R, uint32_t NS, int SRC, int DST, typename Load,
          typename Store>
__device__ __forceinline__ void CPass(Cx<double>* buf, const Cx<double>* t1,
                                      const Cx<double>* t2, uint32_t tid, Load load,
                                      Store store) {
  constexpr uint32_t NB = N / R;
  constexpr uint32_t BPT = (NB + TH - 1) / TH;
  Cx<double> v[BPT][R];
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
#pragma unroll
      for (uint32_t r = 0; r < R; ++r)
        v[i][r] = SRC == 0 ? buf[j + r * NB] : load(j + r * NB);
    }
  }
  if constexpr (SRC == 0) LdsSync();  // every read done before any write
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t j = tid + i * TH;
    if (NB % TH == 0 || j < NB) {
      const uint32_t k = j % NS;
      if constexpr (NS > 1) {
        const uint32_t e = k * (N / (NS * R));
        const Cx<double> w = Mul(t1[e >> kTwShift], t2[e & (kTwLo - 1u)]);
        Cx<double> wr = w;
        v[i][1] = Mul(v[i][1], wr);
#pragma unroll
        for (uint32_t r = 2; r < R; ++r) {
          wr = Mul(wr, w);
          v[i][r] = Mul(v[i][r], wr);
        }
      }
      Dft<double, int(R)>::Run(v[i]);
      const uint32_t d = (j / NS) * NS * R + k;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) store(i, r, d + r * NS, v[i][r]);
    }
  }
  if constexpr (DST == 0) LdsSync();
}

// passes 2 .. of the forward transform (LDS to LDS); the last one goes
// through `last` (the K multiply)
template <uint32_t TH, uint32_t N, uint32_t NS, typename Last, uint32_t R, uint32_t... Rest>
__device__ __forceinline__ void CFwdTail(Cx<double>* buf, const Cx<double>* t1,
                                         const Cx<double>* t2, uint32_t tid, Last last) {
  auto nop = [](uint32_t) { return Cx<double>{0.0, 0.0}; };
  if constexpr (sizeof...(Rest) == 0) {
    CPass<TH, N, R, NS, 0, 0>(buf, t1, t2, tid, nop, last);
  } else {
    CPass<TH, N, R, NS, 0, 0>(buf, t1, t2, tid, nop,
                              [&](uint32_t, uint32_t, uint32_t y, Cx<double> v) { buf[y] = v; });
    CFwdTail<TH, N, NS * R, Last, Rest...>(buf, t1, t2, tid, last);
  }
}

// the inverse transform's passes (LDS to LDS, the last one to `last`)
template <uint32_t TH, uint32_t N, uint32_t NS, typename Last, uint32_t R, uint32_t... Rest>
__device__ __forceinline__ void CInv(Cx<double>* buf, const Cx<double>* t1, const Cx<double>* t2,
                                     uint32_t tid, Last last) {
  auto nop = [](uint32_t) { return Cx<double>{0.0, 0.0}; };
  if constexpr (sizeof...(Rest) == 0) {
    CPass<TH, N, R, NS, 0, 1>(buf, t1, t2, tid, nop, last);
  } else {
    CPass<TH, N, R, NS, 0, 0>(buf, t1, t2, tid, nop,
                              [&](uint32_t, uint32_t, uint32_t y, Cx<double> v) { buf[y] = v; });
    CInv<TH, N, NS * R, Last, Rest...>(buf, t1, t2, tid, last);
  }
}

template <uint32_t... Rs>
constexpr uint32_t LastOf() {
  constexpr uint32_t r[] = {Rs...};
  return r[sizeof...(Rs) - 1];
}

// KF: the kernel spectrum stored as float complex (half the bytes of the
// pass's largest read), widened to double where it is multiplied
template <uint32_t TH, bool KF, uint32_t R1, uint32_t... Rs>
__global__ __launch_bounds__(TH) void ColumnsConvD(ColArgs a, const Cx<double>* __restrict__ in,
                                                   Cx<double>* out, const void* __restrict__ kern_v,
                                                   const Cx<double>* __restrict__ tw) {
  using KT = std::conditional_t<KF, Cx<float>, Cx<double>>;
  const KT* __restrict__ kern = static_cast<const KT*>(kern_v);
  constexpr uint32_t N = R1 * Product<Rs...>();
  constexpr uint32_t RL = LastOf<R1, Rs...>();
  constexpr uint32_t NBL = N / RL;  // last pass: butterflies, = its span
  constexpr uint32_t BL = (NBL + TH - 1) / TH;
  constexpr uint32_t NT1 = (N + kTwLo - 1) / kTwLo;
  constexpr uint32_t NWORDS = (N + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<double>* buf = reinterpret_cast<Cx<double>*>(lds_raw);
  Cx<double>* t1 = buf + N;
  Cx<double>* t2 = t1 + NT1;
  uint32_t* bits = reinterpret_cast<uint32_t*>(t2 + kTwLo);
  const uint32_t b = blockIdx.x, G = gridDim.x;
  const double s = a.scale;
  {
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < NT1; i += TH) t1[i] = tw[i * kTwLo];
    for (uint32_t i = tid; i < kTwLo; i += TH) t2[i] = tw[i];
    for (uint32_t i = tid; i < NWORDS; i += TH) bits[i] = 0u;
    __syncthreads();
    // the input's non-zero rows (a list, or a range)
    const bool listed = a.rows != nullptr;
    const uint32_t n_rows = listed ? *a.n_rows : a.row_n;
    for (uint32_t q = tid; q < n_rows; q += TH) {
      const uint32_t y = listed ? a.rows[q] : a.row0 + q;
      if (y < N) atomicOr(&bits[y >> 5], 1u << (y & 31u));
    }
    __syncthreads();
  }
  for (uint32_t round = 0; round * G < a.n_cols; ++round) {
    uint32_t tid = threadIdx.x;  // opaque per round (see Columns)
    asm volatile("" : "+v"(tid));
    const uint32_t c = round * G + (b & 7u) * a.per_xcd + (b >> 3);
    const bool active = c < a.n_cols;
    const uint32_t cc = active ? c : 0u;
    // column c: row-major (stride ld) or tiled (stride kTile in its tile)
    const size_t in_stride = a.tiled ? kTile : a.ld;
    const Cx<double>* in_c =
        in + (a.tiled ? size_t(cc / kTile) * N * kTile + cc % kTile : size_t(cc));
    const uint32_t k_stride = a.kern_cm ? 1u : a.ld;
    const KT* kern_c = a.kern_cm ? kern + size_t(cc) * N : kern + cc;
    auto kload = [&](uint32_t y) {
      const KT k = kern_c[y * k_stride];
      return Cx<double>{double(k.x), double(k.y)};
    };
    // K x s in the last forward pass's output order: rows j + r NBL; held in
    // registers from the round's start (512 threads), or read where it is
    // multiplied (1024 threads: the registers go to the second set of waves)
    // (register K before the forward transform costs more than it hides:
    // the first pass's input loads then wait for it in order, vmcnt; with a
    // float K at 1 024 threads: 623 -> 668 us per 9072^2 pass; the first two
    // rounds' K issued after the first pass instead: 630 -> 758 us, r05)
    constexpr bool KREG = TH <= 512;
    KT K[KREG ? BL : 1][KREG ? RL : 1];
    if constexpr (KREG) {
#pragma unroll
      for (uint32_t i = 0; i < BL; ++i) {
        const uint32_t j = tid + i * TH;
        if (NBL % TH == 0 || j < NBL)
#pragma unroll
          for (uint32_t r = 0; r < RL; ++r) K[i][r] = kern_c[(j + r * NBL) * k_stride];
      }
    }
    // forward pass 1: straight from global memory through the row bitmap
    auto load = [&](uint32_t y) {
      return ((bits[y >> 5] >> (y & 31u)) & 1u) && active ? in_c[size_t(y) * in_stride]
                                                           : Cx<double>{0.0, 0.0};
    };
    CPass<TH, N, R1, 1, 1, 0>(buf, t1, t2, tid, load,
                              [&](uint32_t, uint32_t, uint32_t y, Cx<double> v) { buf[y] = v; });
    auto mulk = [&](uint32_t i, uint32_t r, uint32_t y, Cx<double> v) {
      Cx<double> k;
      if constexpr (KREG)
        k = Cx<double>{double(K[i][r].x), double(K[i][r].y)};
      else
        k = kload(tid + i * TH + r * NBL);
      buf[y] = Conj(Scale(Mul(v, k), s));
    };
    CFwdTail<TH, N, R1, decltype(mulk), Rs...>(buf, t1, t2, tid, mulk);
    // inverse = conj(forward(conj(X K s))); the last pass stores the window rows
    auto store = [&](uint32_t, uint32_t, uint32_t y, Cx<double> v) {
      if (active && y - a.out_row0 < a.out_row_n)
        out[a.tiled ? TileIndex(y, c, N) : a.out_cm ? size_t(c) * N + y : size_t(y) * a.ld + c] =
            Conj(v);
    };
    // (its LDS reads end in a barrier, before the next round's first stores)
    CInv<TH, N, 1, decltype(store), R1, Rs...>(buf, t1, t2, tid, store);
  }
}

}  // namespace ff

#define RDL_CONV_D(TH, ...)                                                    \
  FastColumns {                                                                \
    ff::Product<__VA_ARGS__>(), true, TH,                                      \
        reinterpret_cast<const void*>(&ff::ColumnsConvD<TH, false, __VA_ARGS__>), \
        MakeRadixList<__VA_ARGS__>(),                                          \
        reinterpret_cast<const void*>(&ff::ColumnsConvD<TH, true, __VA_ARGS__>)  \
  }
const FastColumns* FindConvColumnsD(uint32_t n) {
  static const FastColumns kPlans[] = {
      // 1024 threads for the large sizes (one column's 145 KiB of LDS per
      // CU: twice the waves cover the passes' LDS and memory waits; 9072:
      // 779 -> 661 us against 512 threads, tools/bench_fftk.py f64)
      RDL_CONV_D(1024, 7, 9, 9, 4, 4),        // 9072
      RDL_CONV_D(1024, 9, 4, 4, 4, 4, 4),     // 9216
      RDL_CONV_D(1024, 7, 3, 7, 4, 4, 4),     // 9408
      RDL_CONV_D(1024, 7, 5, 3, 5, 3, 3, 2),  // 9450
      RDL_CONV_D(512, 7, 9, 9, 8),           // 4536
      RDL_CONV_D(512, 9, 8, 8, 8),           // 4608
      RDL_CONV_D(512, 7, 3, 7, 8, 4),        // 4704
      RDL_CONV_D(512, 5, 3, 5, 8, 8),        // 4800
      RDL_CONV_D(512, 5, 5, 5, 5, 8),        // 5000
  };
  for (const FastColumns& p : kPlans)
    if (p.n == n) return &p;
  return nullptr;
}
#undef RDL_CONV_D

size_t ConvColumnsDLdsBytes(uint32_t n) {
  return size_t(n) * 16 + size_t((n + ff::kTwLo - 1) / ff::kTwLo + ff::kTwLo) * 16 +
         size_t((n + 31) / 32) * 4;
}

int ConvColumnsDLaunch(rdl_session* s, const FastColumns* p, const void* in, void* out,
                       const void* kern, const void* tw, uint32_t n_cols, int kern_cm,
                       int out_cm, const uint32_t* rows, const uint32_t* n_rows, uint32_t row0,
                       uint32_t row_n, double scale, uint32_t out_row0, uint32_t out_row_n,
                       bool kernel_f32, bool tiled) {
  const size_t lds = ConvColumnsDLdsBytes(p->n);
  const void* fn = kernel_f32 ? p->kernel_kf : p->kernel;
  if (!fn) {
    SetError("float64 correction columns: no float-kernel plan");
    return RDL_ERR_UNSUPPORTED;
  }
  const int slots = SlotsPerCu(s, fn, p->threads, lds);
  if (slots < 0) {
    SetError("float64 correction columns: occupancy query failed");
    return RDL_ERR_HIP;
  }
  ff::ColArgs a{};
  a.n_cols = n_cols;
  a.ld = n_cols;
  a.mode = 1;
  a.kern_cm = kern_cm ? 1u : 0u;
  a.out_cm = out_cm ? 1u : 0u;
  a.rows = rows;
  a.n_rows = n_rows;
  a.row0 = rows ? 0u : row0;
  a.row_n = rows ? p->n : row_n;
  a.scale = scale;
  a.out_row0 = out_row0;
  a.out_row_n = out_row_n;
  a.tiled = tiled ? 1u : 0u;

  const uint32_t want = std::min<uint32_t>(n_cols, uint32_t(s->n_cus) * uint32_t(slots));
  a.per_xcd = std::max<uint32_t>(1, (want + 7) / 8);
  const uint32_t grid = 8 * a.per_xcd;
  void* args[] = {&a, (void*)&in, (void*)&out, (void*)&kern, (void*)&tw};
  RDL_HIP_CHECK(hipLaunchKernel(fn, dim3(grid), dim3(p->threads), args, lds, s->stream));
  return RDL_OK;
}

}  // namespace rdl
