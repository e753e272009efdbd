// The one-pass column kernels of the compile-time-planned FFT engine (see
// fft_fast.hip), their plans and launcher.
#include <algorithm>

#include "fft_fast_internal.h"

namespace rdl {
namespace ff {

// ------------------------------------------------------------- columns
// One spectrum column of length N per workgroup round (persistent grid).
// PF: the kernel column is loaded into registers before the forward
// transform (in flight meanwhile); otherwise after it.
template <typename T, uint32_t TH, bool PF, uint32_t... Rs>
__global__ __launch_bounds__(TH) void Columns(ColArgs a, const Cx<T>* __restrict__ in,
                                              Cx<T>* out,
                                              const Cx<T>* __restrict__ kern,
                                              const Cx<T>* __restrict__ ptw) {
  constexpr uint32_t N = Product<Rs...>();
  constexpr uint32_t E = (N + TH - 1) / TH;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x, G = gridDim.x;
  const T s = T(a.scale);
  // sparse: only some rows are non-zero (a list, or a range short of N);
  // LDS then holds zeros everywhere else between columns
  const bool listed = a.rows != nullptr && a.mode != 2;
  const bool sparse = a.mode != 2 && (listed || a.row_n < N);
  const uint32_t n_rows = listed ? *a.n_rows : a.row_n;
  if (sparse) {
#pragma unroll
    for (uint32_t i = 0; i < E; ++i) {
      const uint32_t y = tid + i * TH;
      if (N % TH == 0 || y < N) buf[Lx<T>(y)] = Cx<T>{T(0), T(0)};
    }
    LdsSync();
  }
  for (uint32_t round = 0; round * G < a.n_cols; ++round) {
    // opaque per round: keeps the (loop-invariant) per-element addresses of
    // every pass from being hoisted out of the loop into spilled registers
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    // XCD-aware: the columns of one round on one XCD are contiguous, so the
    // row-major lines they share meet in one L2
    const uint32_t c = round * G + (b & 7u) * a.per_xcd + (b >> 3);
    const bool active = c < a.n_cols;
    // uniform column bases (scalar registers) + 32-bit element offsets
    const uint32_t in_stride = (a.mode == 2 && a.in_cm) ? 1u : a.ld;
    const Cx<T>* in_c = (a.mode == 2 && a.in_cm) ? in + size_t(c) * N : in + c;
    const uint32_t k_stride = a.kern_cm ? 1u : a.ld;
    const Cx<T>* kern_c = a.kern_cm ? kern + size_t(c) * N : kern + c;
    Cx<T> K[E];
    auto load_kernel = [&]() {
#pragma unroll
      for (uint32_t i = 0; i < E; ++i) {
        const uint32_t y = tid + i * TH;
        if (N % TH == 0 || y < N) K[i] = kern_c[y * k_stride];
      }
    };
    if (active) {
      if (sparse) {
        for (uint32_t q = tid; q < n_rows; q += TH) {
          const uint32_t y = listed ? a.rows[q] : a.row0 + q;
          buf[Lx<T>(y)] = in_c[y * in_stride];
        }
      } else {
#pragma unroll
        for (uint32_t i = 0; i < E; ++i) {
          const uint32_t y = tid + i * TH;
          if (N % TH == 0 || y < N) buf[Lx<T>(y)] = in_c[y * in_stride];
        }
      }
      if (PF && a.mode != 0) load_kernel();
    }
    LdsSync();
    if (a.mode != 2) Fft<T, TH, N, 0, 1, Rs...>(buf, ptw, tid);
    if (a.mode != 0) {
      if (!PF && active) load_kernel();
      // inverse = conj(forward(conj(X K s)))
#pragma unroll
      for (uint32_t i = 0; i < E; ++i) {
        const uint32_t y = tid + i * TH;
        if (N % TH == 0 || y < N) buf[Lx<T>(y)] = Conj(Scale(Mul(buf[Lx<T>(y)], K[i]), s));
      }
      LdsSync();
      Fft<T, TH, N, 0, 1, Rs...>(buf, ptw, tid);
    }
    if (active) {
      const uint32_t o_stride = a.out_cm ? 1u : a.ld;
      Cx<T>* out_c = a.out_cm ? out + size_t(c) * N : out + c;
#pragma unroll
      for (uint32_t i = 0; i < E; ++i) {
        const uint32_t y = tid + i * TH;
        if (N % TH == 0 || y < N) {
          Cx<T> v = buf[Lx<T>(y)];
          if (a.mode != 0) v = Conj(v);
          out_c[y * o_stride] = v;
          if (sparse) buf[Lx<T>(y)] = Cx<T>{T(0), T(0)};
        }
      }
    } else if (sparse) {
#pragma unroll
      for (uint32_t i = 0; i < E; ++i) {
        const uint32_t y = tid + i * TH;
        if (N % TH == 0 || y < N) buf[Lx<T>(y)] = Cx<T>{T(0), T(0)};
      }
    }
    LdsSync();
  }
}

}  // namespace ff

// ---------------------------------------------------------------- plans
// Supported transform lengths: columns (full length N) and rows (half length
// H = N / 2). Radices in pass order; double stays at radix <= 9 and keeps
// each pass's butterflies-per-thread x radix small (1024 threads leave 128
// VGPRs; checked spill-free with -Rpass-analysis=kernel-resource-usage).
#define RDL_FAST_COLS(T, TH, PF, ...)                                          \
  FastColumns {                                                                \
    ff::Product<__VA_ARGS__>(), sizeof(T) == 8, TH,                            \
        reinterpret_cast<const void*>(&ff::Columns<T, TH, PF, __VA_ARGS__>),   \
        MakeRadixList<__VA_ARGS__>()                                           \
  }

const FastColumns* FindFastColumns(uint32_t n, bool f64) {
  static const FastColumns kPlans[] = {
      // float64 padded correction sizes of 8192^2 (scales 0..256) and 4096^2
      RDL_FAST_COLS(double, 1024, true, 7, 9, 9, 4, 4),        // 9072
      RDL_FAST_COLS(double, 1024, true, 9, 4, 4, 4, 4, 4),     // 9216
      RDL_FAST_COLS(double, 1024, true, 7, 3, 7, 4, 4, 4),     // 9408
      RDL_FAST_COLS(double, 1024, true, 7, 5, 3, 5, 3, 3, 2),  // 9450
      RDL_FAST_COLS(double, 1024, true, 7, 9, 9, 8),           // 4536
      RDL_FAST_COLS(double, 1024, true, 9, 8, 8, 8),           // 4608
      RDL_FAST_COLS(double, 1024, true, 7, 3, 7, 8, 4),        // 4704
      RDL_FAST_COLS(double, 1024, true, 5, 3, 5, 8, 8),        // 4800
      RDL_FAST_COLS(double, 1024, true, 5, 5, 5, 5, 8),        // 5000
      // float64 padded corrections of gridded runs' subimages
      // (GetConvolutionSize of ~1000-1700 pixel subimages; 1 KiB-36 KiB per
      // column, several workgroups per CU)
      RDL_FAST_COLS(double, 256, true, 7, 5, 5, 3, 2),                 // 1050
      RDL_FAST_COLS(double, 256, true, 5, 9, 3, 8),                    // 1080
      RDL_FAST_COLS(double, 256, true, 7, 5, 8, 4),                    // 1120
      RDL_FAST_COLS(double, 256, true, 7, 9, 9, 2),                    // 1134
      RDL_FAST_COLS(double, 256, true, 9, 8, 4, 4),                    // 1152
      RDL_FAST_COLS(double, 256, true, 7, 7, 3, 8),                    // 1176
      RDL_FAST_COLS(double, 256, true, 5, 5, 3, 4, 4),                 // 1200
      RDL_FAST_COLS(double, 256, true, 5, 5, 5, 5, 2),                 // 1250
      RDL_FAST_COLS(double, 256, true, 7, 5, 9, 4),                    // 1260
      RDL_FAST_COLS(double, 256, true, 5, 8, 8, 4),                    // 1280
      RDL_FAST_COLS(double, 256, true, 9, 9, 4, 4),                    // 1296
      RDL_FAST_COLS(double, 256, true, 7, 3, 8, 8),                    // 1344
      RDL_FAST_COLS(double, 256, true, 7, 7, 7, 4),                    // 1372
      RDL_FAST_COLS(double, 256, true, 7, 5, 5, 8),                    // 1400
      RDL_FAST_COLS(double, 256, true, 5, 9, 8, 4),                    // 1440
      RDL_FAST_COLS(double, 256, true, 9, 9, 9, 2),                    // 1458
      RDL_FAST_COLS(double, 256, true, 7, 7, 5, 3, 2),                 // 1470
      RDL_FAST_COLS(double, 256, true, 5, 5, 5, 3, 4),                 // 1500
      RDL_FAST_COLS(double, 256, true, 7, 9, 3, 8),                    // 1512
      RDL_FAST_COLS(double, 256, true, 3, 8, 8, 8),                    // 1536
      RDL_FAST_COLS(double, 256, true, 7, 7, 8, 4),                    // 1568
      RDL_FAST_COLS(double, 256, true, 5, 9, 9, 4),                    // 1620
      RDL_FAST_COLS(double, 256, true, 7, 5, 3, 4, 4),                 // 1680
      RDL_FAST_COLS(double, 256, true, 7, 5, 9, 3, 2),                 // 1890
      RDL_FAST_COLS(double, 256, true, 5, 3, 8, 8, 2),              // 1920
      RDL_FAST_COLS(double, 256, true, 9, 9, 3, 8),                 // 1944
      RDL_FAST_COLS(double, 256, true, 7, 7, 5, 8),                 // 1960
      RDL_FAST_COLS(double, 256, true, 5, 5, 5, 8, 2),              // 2000
      RDL_FAST_COLS(double, 256, true, 7, 9, 8, 4),                 // 2016
      RDL_FAST_COLS(double, 256, true, 8, 8, 8, 4),                 // 2048
      RDL_FAST_COLS(double, 256, true, 7, 5, 5, 3, 4),              // 2100
      RDL_FAST_COLS(double, 256, true, 5, 9, 3, 8, 2),              // 2160
      RDL_FAST_COLS(double, 256, true, 7, 5, 8, 8),                 // 2240
      RDL_FAST_COLS(double, 256, true, 5, 5, 5, 9, 2),              // 2250
      RDL_FAST_COLS(double, 256, true, 7, 9, 9, 4),                 // 2268
      RDL_FAST_COLS(double, 256, true, 9, 8, 8, 4),                 // 2304
      RDL_FAST_COLS(double, 256, true, 7, 7, 3, 8, 2),              // 2352
      RDL_FAST_COLS(double, 256, true, 5, 5, 3, 8, 4),              // 2400
      RDL_FAST_COLS(double, 256, true, 5, 9, 9, 3, 2),              // 2430
      RDL_FAST_COLS(double, 256, true, 7, 7, 5, 5, 2),              // 2450
      RDL_FAST_COLS(double, 256, true, 5, 5, 5, 5, 4),              // 2500
      RDL_FAST_COLS(double, 256, true, 7, 5, 9, 8),                 // 2520
      RDL_FAST_COLS(double, 256, true, 5, 8, 8, 8),                 // 2560
      RDL_FAST_COLS(double, 256, true, 9, 9, 8, 4),                 // 2592
      RDL_FAST_COLS(double, 256, true, 7, 7, 9, 3, 2),              // 2646
      RDL_FAST_COLS(double, 256, true, 7, 3, 8, 8, 2),              // 2688
      RDL_FAST_COLS(double, 256, true, 7, 7, 7, 8),                 // 2744
      RDL_FAST_COLS(double, 256, true, 7, 5, 5, 8, 2),              // 2800
      RDL_FAST_COLS(double, 256, true, 5, 9, 8, 8),                 // 2880
      RDL_FAST_COLS(double, 256, true, 9, 9, 9, 4),                 // 2916
      RDL_FAST_COLS(double, 256, true, 7, 7, 5, 3, 4),              // 2940
      RDL_FAST_COLS(double, 256, true, 5, 5, 5, 3, 8),              // 3000
      RDL_FAST_COLS(double, 256, true, 7, 9, 3, 8, 2),              // 3024
      RDL_FAST_COLS(double, 256, true, 3, 8, 8, 8, 2),              // 3072
      RDL_FAST_COLS(double, 256, true, 7, 7, 8, 8),                 // 3136
      RDL_FAST_COLS(double, 256, true, 7, 5, 5, 9, 2),              // 3150
      RDL_FAST_COLS(double, 256, true, 5, 5, 8, 8, 2),              // 3200
      RDL_FAST_COLS(double, 256, true, 5, 9, 9, 8),                 // 3240
      RDL_FAST_COLS(double, 256, true, 7, 5, 3, 8, 4),              // 3360
      RDL_FAST_COLS(double, 256, true, 7, 9, 9, 3, 2),              // 3402
      RDL_FAST_COLS(double, 256, true, 7, 7, 7, 5, 2),              // 3430
      RDL_FAST_COLS(double, 256, true, 7, 5, 5, 5, 4),              // 3500
      // float32 scale convolutions (two workgroups per CU)
      RDL_FAST_COLS(float, 512, true, 8, 8, 8, 16),            // 8192
      RDL_FAST_COLS(float, 512, true, 8, 8, 8, 8),             // 4096
      // the periodically extended subimage planes of a tiled run
      // (MultiScaleTransforms' CanonicalFftSize ladder)
      RDL_FAST_COLS(float, 512, true, 8, 8, 8, 7),             // 3584
      RDL_FAST_COLS(float, 512, true, 8, 8, 16, 3),            // 3072
      RDL_FAST_COLS(float, 512, true, 8, 8, 8, 5),             // 2560
      RDL_FAST_COLS(float, 512, true, 8, 8, 8, 4),             // 2048
      RDL_FAST_COLS(float, 512, true, 8, 8, 4, 7),             // 1792
      RDL_FAST_COLS(float, 512, true, 8, 8, 8, 3),             // 1536
      RDL_FAST_COLS(float, 512, true, 8, 8, 4, 5),             // 1280
  };
  for (const FastColumns& p : kPlans)
    if (p.n == n && p.f64 == f64) return &p;
  return nullptr;
}

#undef RDL_FAST_COLS

int FastColumnsLaunch(rdl_session* s, const FastColumns* p, const void* in, void* out,
                      const void* kern, const void* ptw, uint32_t n_cols, uint32_t mode,
                      int in_cm, int out_cm, int kern_cm, const uint32_t* rows,
                      const uint32_t* n_rows, uint32_t row0, uint32_t row_n,
                      double scale) {
  const size_t lds = FastLdsBytes(p->n, p->f64);
  const int slots = SlotsPerCu(s, p->kernel, p->threads, lds);
  if (slots < 0) {
    SetError("fast FFT columns: occupancy query failed");
    return RDL_ERR_HIP;
  }
  ff::ColArgs a{};
  a.n_cols = n_cols;
  a.ld = n_cols;
  a.mode = mode;
  a.in_cm = in_cm ? 1u : 0u;
  a.out_cm = out_cm ? 1u : 0u;
  a.kern_cm = kern_cm ? 1u : 0u;
  a.rows = rows;
  a.n_rows = n_rows;
  a.row0 = rows ? 0u : row0;
  a.row_n = rows ? p->n : row_n;
  a.scale = scale;
  const uint32_t want = std::min<uint32_t>(n_cols, uint32_t(s->n_cus) * uint32_t(slots));
  a.per_xcd = std::max<uint32_t>(1, (want + 7) / 8);
  const uint32_t grid = 8 * a.per_xcd;
  void* args[] = {&a, (void*)&in, (void*)&out, (void*)&kern, (void*)&ptw};
  RDL_HIP_CHECK(hipLaunchKernel(p->kernel, dim3(grid), dim3(p->threads), args, lds,
                                s->stream));
  return RDL_OK;
}

}  // namespace rdl
