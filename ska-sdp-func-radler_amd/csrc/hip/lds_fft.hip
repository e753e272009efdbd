// LDS-resident FFT convolution engine: the multiscale scale convolutions and
// SubMinorLoop::CorrectResidualDirty (cpp/algorithms/multiscale/
// multiscale_transforms.cc:9-21, cpp/algorithms/subminor_loop.cc:195-218;
// schaapcommon::math::Convolve contract restated in oracle/oracle.cc) as
// three HBM passes instead of rocFFT's transpose-heavy plans:
//
//   rows forward   : two real rows per transform packed as z = a + i b, one
//                    complex Stockham FFT of the row length in LDS, split into
//                    the two half spectra (W/2+1 bins) -> row-major spectrum.
//                    The input is read from a w x h float image placed at an
//                    offset inside the (possibly padded) plane (Image::Untrim
//                    fused; rows outside it are zero and never loaded).
//   columns        : `count` spectrum columns per workgroup, complex FFT of the
//                    column length in LDS; optionally x kernel spectrum x 1/N
//                    and the inverse column FFT in the same pass.
//   rows inverse   : Hermitian half rows -> packed complex row -> inverse FFT
//                    in LDS -> two real rows, written (Image::Trim fused) or
//                    subtracted from the residual.
//
// Lengths must be 2^a 3^b 5^c 7^d (every CalculateGoodFFTSize output is) and
// fit one workgroup (kMaxWgElems = 10240 complex elements in either precision;
// in double that is all 160 KiB of LDS); otherwise
// rdl_conv_create returns RDL_ERR_UNSUPPORTED and callers use rocFFT.
// Twiddles come from a float64 table (rounded to T for float plans).
//
// These are the runtime-plan kernels: one kernel per pass and precision, the
// radices read from the plan. conv.hip owns the rdl_conv object and chooses
// per call between them and the compile-time plans of fft_fast*.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fft_dft.h"
#include "lds_fft.h"
#include "rdl_internal.h"

namespace rdl {

// ---- one Stockham pass over `count` transforms of length n held in LDS
// (in place: all butterfly inputs are read to registers before the barrier)
// Not inlined on purpose: with every radix inlined into one kernel the
// register allocator spilled 150-300 bytes per lane (scratch traffic showed
// up as 4-5x the algorithmic HBM writes); as separate functions each pass is
// allocated on its own (no spills; the call saves a few callee-saved VGPRs).
template <typename T, int R>
__device__ __attribute__((noinline)) void StockhamPass(Cx<T>* buf, uint32_t n,
                                             uint32_t count, uint32_t ns,
                                             const Cx<T>* __restrict__ tw,
                                             uint32_t tid, uint32_t stride) {
  constexpr uint32_t BPT = StockhamBpt(R);
  const uint32_t nb = n / R;
  const uint32_t total = nb * count;
  const uint32_t m = n / (ns * R);
  Cx<T> v[BPT][R];
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t b = tid + i * kFftThreads;
    if (b < total) {
      const uint32_t t = b / nb, j = b - t * nb;
      const Cx<T>* base = buf + size_t(t) * stride;
#pragma unroll
      for (int r = 0; r < R; ++r) v[i][r] = base[j + r * nb];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t i = 0; i < BPT; ++i) {
    const uint32_t b = tid + i * kFftThreads;
    if (b < total) {
      const uint32_t t = b / nb, j = b - t * nb;
      const uint32_t k = j % ns;
      if (ns > 1) {
#pragma unroll
        for (int r = 1; r < R; ++r) v[i][r] = Mul(v[i][r], tw[k * r * m]);
      }
      Dft<T, R>::Run(v[i]);
      Cx<T>* base = buf + size_t(t) * stride;
      const uint32_t d = (j / ns) * ns * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) base[d + r * ns] = v[i][r];
    }
  }
  __syncthreads();
}

// Forward complex FFT (natural order in and out) of `count` transforms, each
// `stride` elements apart (>= n; padding keeps transposing loads off one bank).
template <typename T>
__device__ void LdsFftForward(Cx<T>* buf, const LdsPlan& p, uint32_t count,
                              uint32_t tid, uint32_t stride = 0) {
  if (stride == 0) stride = p.n;
  const Cx<T>* tw = static_cast<const Cx<T>*>(p.tw);
  uint32_t ns = 1;
  for (uint32_t q = 0; q < p.n_pass; ++q) {
    const uint32_t r = p.radix[q];
    switch (r) {
      case 16:
        if constexpr (sizeof(T) == 4) StockhamPass<T, 16>(buf, p.n, count, ns, tw, tid, stride);
        break;
      case 9:
        if constexpr (sizeof(T) == 4) StockhamPass<T, 9>(buf, p.n, count, ns, tw, tid, stride);
        break;
      case 8: StockhamPass<T, 8>(buf, p.n, count, ns, tw, tid, stride); break;
      case 4: StockhamPass<T, 4>(buf, p.n, count, ns, tw, tid, stride); break;
      case 2: StockhamPass<T, 2>(buf, p.n, count, ns, tw, tid, stride); break;
      case 3: StockhamPass<T, 3>(buf, p.n, count, ns, tw, tid, stride); break;
      case 5: StockhamPass<T, 5>(buf, p.n, count, ns, tw, tid, stride); break;
      default: StockhamPass<T, 7>(buf, p.n, count, ns, tw, tid, stride); break;
    }
    ns *= r;
  }
}

// ---------------------------------------------------------------- kernels
struct RowArgs {
  LdsPlan plan;        // row length n = plane width
  uint32_t height;     // plane rows
  uint32_t count;      // row pairs per workgroup
  uint32_t ld;         // spectrum row stride (complex) = n/2+1
  // forward input / inverse output window inside the plane
  uint32_t img_w, img_h, ox, oy;
  // forward: per plane row, 0 = known zero. A workgroup whose rows are all
  // zero neither reads nor writes (the column pass must get the same mask)
  const uint8_t* row_mask;
};

// rows forward: float image window -> half spectra (T)
template <typename T>
__global__ __launch_bounds__(kFftThreads) void RowsForward(RowArgs a,
                                                           const float* __restrict__ in,
                                                           Cx<T>* __restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  const uint32_t tid = threadIdx.x;
  const uint32_t n = a.plan.n;
  const uint32_t pair0 = blockIdx.x * a.count;
  const uint32_t n_pairs = (a.height + 1) / 2;
  const uint32_t count = min(a.count, n_pairs - pair0);
  if (a.row_mask) {
    // workgroup OR through the (not yet used) dynamic LDS: the engine owns
    // all of it, so no static __shared__ flag or __syncthreads_or
    volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(lds_raw);
    if (tid == 0) *flag = 0u;
    __syncthreads();
    const uint32_t y = 2 * pair0 + tid;
    if (tid < 2 * count && y < a.height && a.row_mask[y] != 0) *flag = 1u;
    __syncthreads();
    const bool any = *flag != 0u;
    __syncthreads();
    if (!any) return;
  }
  for (uint32_t idx = tid; idx < count * n; idx += kFftThreads) {
    const uint32_t t = idx / n, x = idx - t * n;
    const uint32_t y0 = 2 * (pair0 + t), y1 = y0 + 1;
    T va = T(0), vb = T(0);
    const int64_t ix = int64_t(x) - a.ox;
    // A masked row is zero whatever the plane holds there: the two rows of a
    // pair share one complex transform, so a stale row would leak into its
    // partner's spectrum through rounding (the partial-zeroing correction
    // model plane keeps old data in its unmarked rows).
    const bool use0 = !a.row_mask || a.row_mask[y0] != 0;
    const bool use1 = y1 < a.height && (!a.row_mask || a.row_mask[y1] != 0);
    if (ix >= 0 && ix < a.img_w) {
      const int64_t iy0 = int64_t(y0) - a.oy, iy1 = int64_t(y1) - a.oy;
      if (use0 && iy0 >= 0 && iy0 < a.img_h) va = T(in[size_t(iy0) * a.img_w + ix]);
      if (use1 && iy1 >= 0 && iy1 < a.img_h) vb = T(in[size_t(iy1) * a.img_w + ix]);
    }
    buf[idx] = {va, vb};
  }
  __syncthreads();
  LdsFftForward<T>(buf, a.plan, count, tid);
  const uint32_t nh = n / 2 + 1;
  for (uint32_t idx = tid; idx < count * nh; idx += kFftThreads) {
    const uint32_t t = idx / nh, k = idx - t * nh;
    const Cx<T> zk = buf[size_t(t) * n + k];
    const Cx<T> zc = Conj(buf[size_t(t) * n + (k == 0 ? 0 : n - k)]);
    const T h = T(0.5);
    const Cx<T> A = {h * (zk.x + zc.x), h * (zk.y + zc.y)};
    const Cx<T> B = {h * (zk.y - zc.y), -h * (zk.x - zc.x)};
    const uint32_t y0 = 2 * (pair0 + t), y1 = y0 + 1;
    spec[size_t(y0) * a.ld + k] = A;
    if (y1 < a.height) spec[size_t(y1) * a.ld + k] = B;
  }
}

// rows inverse: half spectra -> real rows; write (mode 0) or subtract
// (mode 1) the window [ox, ox+img_w) x [oy, oy+img_h) into out (img_w wide)
template <typename T>
__global__ __launch_bounds__(kFftThreads) void RowsInverse(RowArgs a,
                                                           const Cx<T>* __restrict__ spec,
                                                           float* __restrict__ out,
                                                           int subtract) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  const uint32_t tid = threadIdx.x;
  const uint32_t n = a.plan.n;
  const uint32_t pair0 = blockIdx.x * a.count;
  const uint32_t n_pairs = (a.height + 1) / 2;
  const uint32_t count = min(a.count, n_pairs - pair0);
  const uint32_t nh = n / 2 + 1;
  const bool even = (n & 1u) == 0;
  for (uint32_t idx = tid; idx < count * nh; idx += kFftThreads) {
    const uint32_t t = idx / nh, k = idx - t * nh;
    const uint32_t y0 = 2 * (pair0 + t), y1 = y0 + 1;
    Cx<T> A = spec[size_t(y0) * a.ld + k];
    Cx<T> B = y1 < a.height ? spec[size_t(y1) * a.ld + k] : Cx<T>{T(0), T(0)};
    if (k == 0 || (even && k == n / 2)) {  // C2R ignores these imaginary parts
      A.y = T(0);
      B.y = T(0);
    }
    // Z[k] = A + iB ; Z[n-k] = conj(A) + i conj(B). Stored conjugated (inverse
    // FFT = conj(FFT(conj)))
    Cx<T>* row = buf + size_t(t) * n;
    row[k] = {A.x - B.y, -(A.y + B.x)};
    if (k != 0 && !(even && k == n / 2)) row[n - k] = {A.x + B.y, -(B.x - A.y)};
  }
  __syncthreads();
  LdsFftForward<T>(buf, a.plan, count, tid);
  for (uint32_t idx = tid; idx < count * n; idx += kFftThreads) {
    const uint32_t t = idx / n, x = idx - t * n;
    const int64_t ix = int64_t(x) - a.ox;
    if (ix < 0 || ix >= a.img_w) continue;
    const Cx<T> z = buf[idx];  // conj(result): a = z.x, b = -z.y
    const uint32_t y0 = 2 * (pair0 + t), y1 = y0 + 1;
    const int64_t iy0 = int64_t(y0) - a.oy, iy1 = int64_t(y1) - a.oy;
    if (iy0 >= 0 && iy0 < a.img_h) {
      float* o = out + size_t(iy0) * a.img_w + ix;
      if (subtract)
        *o -= float(z.x);
      else
        *o = float(z.x);
    }
    if (y1 < a.height && iy1 >= 0 && iy1 < a.img_h) {
      float* o = out + size_t(iy1) * a.img_w + ix;
      if (subtract)
        *o -= float(-z.y);
      else
        *o = float(-z.y);
    }
  }
}

struct ColArgs {
  LdsPlan plan;      // column length n = plane height
  uint32_t n_cols;   // spectrum columns = width/2+1
  uint32_t count;    // columns per workgroup
  uint32_t ld;       // spectrum row stride
  uint32_t tiles_per_xcd;
  int mode;          // 0 fwd, 1 fwd*K*s+inv, 2 (already fwd) *K*s+inv
  double scale;
  const uint8_t* row_mask;  // rows known zero are not read (NULL: dense)
  uint32_t kern_cm;         // kernel spectrum column-major (column k at k*n)
  uint32_t out_cm;          // mode 0: write the spectrum column-major
};

template <typename T>
__global__ __launch_bounds__(kFftThreads) void Columns(ColArgs a,
                                                       const Cx<T>* __restrict__ in,
                                                       Cx<T>* __restrict__ out,
                                                       const Cx<T>* __restrict__ kern) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  // XCD-aware tiles: consecutive column tiles run on the same XCD so the
  // 128-byte lines they share are fetched into one L2
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  const uint32_t tile = xcd * a.tiles_per_xcd + slot;
  const uint32_t k0 = tile * a.count;
  if (k0 >= a.n_cols) return;
  const uint32_t count = min(a.count, a.n_cols - k0);
  const uint32_t tid = threadIdx.x;
  const uint32_t n = a.plan.n;
  const T s = T(a.scale);
  for (uint32_t idx = tid; idx < count * n; idx += kFftThreads) {
    const uint32_t y = idx / count, j = idx - y * count;
    Cx<T> v = (a.row_mask && a.row_mask[y] == 0) ? Cx<T>{T(0), T(0)}
                                                 : in[size_t(y) * a.ld + k0 + j];
    if (a.mode == 2)
      v = Conj(Scale(Mul(v, a.kern_cm ? kern[size_t(k0 + j) * n + y]
                                      : kern[size_t(y) * a.ld + k0 + j]),
                     s));
    buf[size_t(j) * n + y] = v;
  }
  __syncthreads();
  if (a.mode != 2) LdsFftForward<T>(buf, a.plan, count, tid);
  if (a.mode == 1) {
    if (a.kern_cm) {  // contiguous kernel columns: walk each column
      for (uint32_t idx = tid; idx < count * n; idx += kFftThreads) {
        Cx<T>& v = buf[idx];  // idx = j*n + y
        v = Conj(Scale(Mul(v, kern[size_t(k0) * n + idx]), s));
      }
    } else {
      for (uint32_t idx = tid; idx < count * n; idx += kFftThreads) {
        const uint32_t y = idx / count, j = idx - y * count;
        Cx<T>& v = buf[size_t(j) * n + y];
        v = Conj(Scale(Mul(v, kern[size_t(y) * a.ld + k0 + j]), s));
      }
    }
    __syncthreads();
  }
  if (a.mode != 0) LdsFftForward<T>(buf, a.plan, count, tid);
  if (a.out_cm) {  // column-major spectrum (mode 0 only)
    for (uint32_t idx = tid; idx < count * n; idx += kFftThreads)
      out[size_t(k0) * n + idx] = buf[idx];
    return;
  }
  for (uint32_t idx = tid; idx < count * n; idx += kFftThreads) {
    const uint32_t y = idx / count, j = idx - y * count;
    const Cx<T> v = buf[size_t(j) * n + y];
    out[size_t(y) * a.ld + k0 + j] = a.mode == 0 ? v : Conj(v);
  }
}

// ------------------------------------------- split (four-step) column passes
// A column transform of length N = N1 * N2 in two coalesced passes instead of
// one strided one (with one double column per workgroup the single-pass
// column kernel touches a separate 128-byte line for every element):
//   A  : for each n2, the N1 elements at rows N2*n1 + n2 (strided rows, but
//        `cols` adjacent columns per row, so every load/store is a full
//        line): length-N1 FFT, x W_N^(n2*k1), back to rows N2*k1 + n2.
//   B  : for each k1, the N2 elements at rows N2*k1 + n2 (one contiguous
//        block of rows): length-N2 FFT -> X[k1 + N1*k2].
// The inverse runs the same passes backwards (B^-1 over the block, then A^-1
// with conj twiddles). B stores/loads the spectrum in natural row order
// (row k1 + N1*k2), so spectra keep the single-pass layout; the fused
// convolution (forward, x K x s, inverse) keeps B and B^-1 in one pass over
// the block.
struct SplitArgs {
  LdsPlan plan;        // sub-transform (N1 for A, N2 for B)
  uint32_t n, n1, n2;  // column length and its split
  uint32_t n_cols;     // spectrum columns (W/2+1)
  uint32_t ld;         // spectrum row stride
  uint32_t cols;       // adjacent columns per tile
  uint32_t groups;     // sub-columns per tile (A: n2 values, B: k1 values)
  uint32_t col_tiles;  // tiles across the columns
  uint32_t n_groups;   // A: n2, B: n1
  const void* tw_n;    // exp(-2 pi i k / N), k < N
  const uint8_t* row_mask;  // A forward: rows known zero are not read
  double scale;
  int mode;            // A: 0 forward, 1 inverse. B: 0 fwd, 1 fwd*K*s+inv, 2 *K*s+inv
};

template <typename T>
__global__ __launch_bounds__(kFftThreads) void ColumnsSplitA(SplitArgs a,
                                                             const Cx<T>* in,
                                                             Cx<T>* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  const uint32_t ct = blockIdx.x % a.col_tiles, gt = blockIdx.x / a.col_tiles;
  const uint32_t k0 = ct * a.cols, g0 = gt * a.groups;
  const uint32_t cnt = min(a.cols, a.n_cols - k0);
  const uint32_t gcnt = min(a.groups, a.n_groups - g0);
  const uint32_t tid = threadIdx.x, n1 = a.n1, n2 = a.n2, C = a.cols;
  const bool inverse = a.mode == 1;
  const Cx<T>* __restrict__ twn = static_cast<const Cx<T>*>(a.tw_n);
  const uint32_t total = n1 * gcnt * C;
  for (uint32_t idx = tid; idx < total; idx += kFftThreads) {
    const uint32_t j = idx % C, rest = idx / C;
    const uint32_t g = rest % gcnt, i1 = rest / gcnt;
    const uint32_t sub = g0 + g;
    const uint32_t row = n2 * i1 + sub;
    Cx<T> v{T(0), T(0)};
    if (j < cnt && !(a.row_mask && a.row_mask[row] == 0))
      v = in[size_t(row) * a.ld + k0 + j];
    if (inverse)  // conj(v * conj(w)) = conj(v) * w, w = W_N^(n2*k1)
      v = Mul(Conj(v), twn[(uint64_t(sub) * i1) % a.n]);
    buf[size_t(g * C + j) * (n1 + 1) + i1] = v;
  }
  __syncthreads();
  LdsFftForward<T>(buf, a.plan, gcnt * C, tid, n1 + 1);
  for (uint32_t idx = tid; idx < total; idx += kFftThreads) {
    const uint32_t j = idx % C, rest = idx / C;
    const uint32_t g = rest % gcnt, i1 = rest / gcnt;
    const uint32_t sub = g0 + g;
    Cx<T> v = buf[size_t(g * C + j) * (n1 + 1) + i1];
    v = inverse ? Conj(v) : Mul(v, twn[(uint64_t(sub) * i1) % a.n]);
    if (j < cnt) out[size_t(n2 * i1 + sub) * a.ld + k0 + j] = v;
  }
}

template <typename T>
__global__ __launch_bounds__(kFftThreads) void ColumnsSplitB(SplitArgs a,
                                                             const Cx<T>* in,
                                                             Cx<T>* out,
                                                             const Cx<T>* kern) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  Cx<T>* buf = reinterpret_cast<Cx<T>*>(lds_raw);
  const uint32_t ct = blockIdx.x % a.col_tiles, gt = blockIdx.x / a.col_tiles;
  const uint32_t k0 = ct * a.cols, g0 = gt * a.groups;
  const uint32_t cnt = min(a.cols, a.n_cols - k0);
  const uint32_t gcnt = min(a.groups, a.n_groups - g0);
  const uint32_t tid = threadIdx.x, n1 = a.n1, n2 = a.n2, C = a.cols;
  const T s = T(a.scale);
  const uint32_t total = n2 * gcnt * C;
  // mode 0/1 read the block (rows n2*k1 + i2), mode 2 the natural spectrum
  // (rows k1 + n1*k2); mode 2 starts in the conjugated domain
  for (uint32_t idx = tid; idx < total; idx += kFftThreads) {
    const uint32_t j = idx % C, rest = idx / C;
    const uint32_t g = rest % gcnt, i2 = rest / gcnt;
    const uint32_t k1 = g0 + g;
    Cx<T> v{T(0), T(0)};
    if (a.mode == 2) {
      const size_t at = size_t(k1 + n1 * i2) * a.ld + k0 + j;
      if (j < cnt) v = Conj(Scale(Mul(in[at], kern[at]), s));
    } else if (j < cnt) {
      v = in[size_t(n2 * k1 + i2) * a.ld + k0 + j];
    }
    buf[size_t(g * C + j) * (n2 + 1) + i2] = v;
  }
  __syncthreads();
  LdsFftForward<T>(buf, a.plan, gcnt * C, tid, n2 + 1);
  if (a.mode == 1) {
    for (uint32_t idx = tid; idx < total; idx += kFftThreads) {
      const uint32_t j = idx % C, rest = idx / C;
      const uint32_t g = rest % gcnt, i2 = rest / gcnt;
      const uint32_t k1 = g0 + g;
      Cx<T>& v = buf[size_t(g * C + j) * (n2 + 1) + i2];
      const Cx<T> k = j < cnt ? kern[size_t(k1 + n1 * i2) * a.ld + k0 + j]
                              : Cx<T>{T(0), T(0)};
      v = Conj(Scale(Mul(v, k), s));
    }
    __syncthreads();
    LdsFftForward<T>(buf, a.plan, gcnt * C, tid, n2 + 1);
  }
  for (uint32_t idx = tid; idx < total; idx += kFftThreads) {
    const uint32_t j = idx % C, rest = idx / C;
    const uint32_t g = rest % gcnt, i2 = rest / gcnt;
    const uint32_t k1 = g0 + g;
    const Cx<T> v = buf[size_t(g * C + j) * (n2 + 1) + i2];
    if (j >= cnt) continue;
    if (a.mode == 0)  // X[k1 + n1*k2] in natural order
      out[size_t(k1 + n1 * i2) * a.ld + k0 + j] = v;
    else  // back from the conjugated domain, block layout for A^-1
      out[size_t(n2 * k1 + i2) * a.ld + k0 + j] = Conj(v);
  }
}

// ---------------------------------------------------------------- planning
// (the radix sequence: Factorize, lds_fft_plan.h)
int MakeLdsPlan(rdl_session* s, uint32_t n, bool f64, LdsPlan* plan, void** tw) {
  std::vector<uint8_t> radix;
  if (!Factorize(n, f64, radix)) {
    SetError("LDS FFT: length " + std::to_string(n) + " is not 2/3/5/7-smooth");
    return RDL_ERR_UNSUPPORTED;
  }
  plan->n = n;
  plan->n_pass = uint32_t(radix.size());
  std::memset(plan->radix, 0, sizeof(plan->radix));
  for (size_t i = 0; i < radix.size(); ++i) plan->radix[i] = radix[i];
  const size_t esz = f64 ? 16 : 8;
  std::vector<unsigned char> host(size_t(n) * esz);
  for (uint32_t k = 0; k < n; ++k) {
    // exp(-2 pi i k/n) with the angle reduced to the first octant in double
    const long double ang = -2.0L * 3.14159265358979323846264338327950288L * k / n;
    const double cr = double(std::cos(ang)), ci = double(std::sin(ang));
    if (f64) {
      double v[2] = {cr, ci};
      std::memcpy(&host[k * esz], v, 16);
    } else {
      float v[2] = {float(cr), float(ci)};
      std::memcpy(&host[k * esz], v, 8);
    }
  }
  RDL_HIP_CHECK(DevMalloc(tw, host.size()));
  RDL_HIP_CHECK(UploadSync(*tw, host.data(), host.size(), s->stream));
  plan->tw = *tw;
  return RDL_OK;
}

// ---------------------------------------------------------------- launches
namespace {

template <typename T>
int RowsForwardT(rdl_session* s, const RowArgs& a, const float* in, void* spec) {
  const uint32_t n_pairs = (a.height + 1) / 2;
  const uint32_t grid = (n_pairs + a.count - 1) / a.count;
  const size_t lds = size_t(a.count) * a.plan.n * sizeof(Cx<T>);
  auto k = RowsForward<T>;
  static std::atomic<uint64_t> attr_done{0};  // per instantiation and device
  RDL_TRY(SetMaxLdsOnce(reinterpret_cast<const void*>(k), int(kFftLdsBytes), s->device,
                        attr_done));
  k<<<grid, kFftThreads, lds, s->stream>>>(a, in, static_cast<Cx<T>*>(spec));
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

template <typename T>
int RowsInverseT(rdl_session* s, const RowArgs& a, const void* spec, float* out,
                 int subtract) {
  const uint32_t n_pairs = (a.height + 1) / 2;
  const uint32_t grid = (n_pairs + a.count - 1) / a.count;
  const size_t lds = size_t(a.count) * a.plan.n * sizeof(Cx<T>);
  auto k = RowsInverse<T>;
  static std::atomic<uint64_t> attr_done{0};  // per instantiation and device
  RDL_TRY(SetMaxLdsOnce(reinterpret_cast<const void*>(k), int(kFftLdsBytes), s->device,
                        attr_done));
  k<<<grid, kFftThreads, lds, s->stream>>>(a, static_cast<const Cx<T>*>(spec), out, subtract);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

template <typename T>
int ColumnsT(rdl_session* s, ColArgs a, const void* in, void* out, const void* kern) {
  const uint32_t n_tiles = (a.n_cols + a.count - 1) / a.count;
  a.tiles_per_xcd = (n_tiles + 7) / 8;
  const uint32_t grid = 8 * a.tiles_per_xcd;
  const size_t lds = size_t(a.count) * a.plan.n * sizeof(Cx<T>);
  auto k = Columns<T>;
  static std::atomic<uint64_t> attr_done{0};  // per instantiation and device
  RDL_TRY(SetMaxLdsOnce(reinterpret_cast<const void*>(k), int(kFftLdsBytes), s->device,
                        attr_done));
  k<<<grid, kFftThreads, lds, s->stream>>>(a, static_cast<const Cx<T>*>(in),
                                           static_cast<Cx<T>*>(out),
                                           static_cast<const Cx<T>*>(kern));
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

// one A or B pass over the whole spectrum
template <typename T>
int ColumnsSplitT(rdl_session* s, const SplitArgs& a, uint32_t grid, size_t lds, bool pass_b,
                  const void* in, void* out, const void* kern) {
  if (pass_b) {
    auto k = ColumnsSplitB<T>;
    static std::atomic<uint64_t> attr_done{0};
    RDL_TRY(SetMaxLdsOnce(reinterpret_cast<const void*>(k), int(kFftLdsBytes), s->device,
                          attr_done));
    k<<<grid, kFftThreads, lds, s->stream>>>(a, static_cast<const Cx<T>*>(in),
                                             static_cast<Cx<T>*>(out),
                                             static_cast<const Cx<T>*>(kern));
  } else {
    auto k = ColumnsSplitA<T>;
    static std::atomic<uint64_t> attr_done{0};
    RDL_TRY(SetMaxLdsOnce(reinterpret_cast<const void*>(k), int(kFftLdsBytes), s->device,
                          attr_done));
    k<<<grid, kFftThreads, lds, s->stream>>>(a, static_cast<const Cx<T>*>(in),
                                             static_cast<Cx<T>*>(out));
  }
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

RowArgs MakeRowArgs(const LdsPlan& plan, uint32_t count, uint32_t height, uint32_t img_w,
                    uint32_t img_h, uint32_t ox, uint32_t oy, const uint8_t* row_mask) {
  RowArgs a{};
  a.plan = plan;
  a.height = height;
  a.count = count;
  a.ld = plan.n / 2 + 1;
  a.img_w = img_w;
  a.img_h = img_h;
  a.ox = ox;
  a.oy = oy;
  a.row_mask = row_mask;
  return a;
}

}  // namespace

int LdsRowsForwardLaunch(rdl_session* s, const LdsPlan& plan, bool f64, uint32_t count,
                         uint32_t height, const float* in, uint32_t img_w, uint32_t img_h,
                         uint32_t ox, uint32_t oy, void* spec, const uint8_t* row_mask) {
  const RowArgs a = MakeRowArgs(plan, count, height, img_w, img_h, ox, oy, row_mask);
  return f64 ? RowsForwardT<double>(s, a, in, spec) : RowsForwardT<float>(s, a, in, spec);
}

int LdsRowsInverseLaunch(rdl_session* s, const LdsPlan& plan, bool f64, uint32_t count,
                         uint32_t height, const void* spec, float* out, uint32_t img_w,
                         uint32_t img_h, uint32_t ox, uint32_t oy, int subtract) {
  const RowArgs a = MakeRowArgs(plan, count, height, img_w, img_h, ox, oy, nullptr);
  return f64 ? RowsInverseT<double>(s, a, spec, out, subtract)
             : RowsInverseT<float>(s, a, spec, out, subtract);
}

int LdsColumnsLaunch(rdl_session* s, const LdsPlan& plan, bool f64, uint32_t count,
                     uint32_t width, const void* in, void* out, const void* kern, int mode,
                     double scale, const uint8_t* row_mask, int kern_cm, int out_cm) {
  ColArgs a{};
  a.row_mask = row_mask;
  a.kern_cm = kern_cm ? 1u : 0u;
  a.out_cm = out_cm ? 1u : 0u;
  a.plan = plan;
  a.n_cols = width / 2 + 1;
  a.count = count;
  a.ld = a.n_cols;
  a.mode = mode;
  a.scale = scale;
  return f64 ? ColumnsT<double>(s, a, in, out, kern) : ColumnsT<float>(s, a, in, out, kern);
}

int LdsColumnsSplitLaunch(rdl_session* s, const LdsSplit& sp, const LdsPlan& col_plan, bool f64,
                          uint32_t width, bool pass_b, int mode, const void* in, void* out,
                          const void* kern, double scale, const uint8_t* row_mask) {
  SplitArgs a{};
  a.plan = pass_b ? sp.plan_n2 : sp.plan_n1;
  a.n = col_plan.n;
  a.n1 = sp.n1;
  a.n2 = sp.n2;
  a.n_cols = width / 2 + 1;
  a.ld = a.n_cols;
  a.cols = sp.cols;
  // the tile geometry: PlanLdsSplitPass, lds_fft_plan.h
  const LdsSplitPass p = PlanLdsSplitPass(sp.n1, sp.n2, sp.cols, f64, width, pass_b);
  a.groups = p.groups;
  a.n_groups = p.n_groups;
  a.col_tiles = p.col_tiles;
  a.tw_n = col_plan.tw;
  a.row_mask = row_mask;
  a.scale = scale;
  a.mode = mode;
  return f64 ? ColumnsSplitT<double>(s, a, p.grid, p.lds, pass_b, in, out, kern)
             : ColumnsSplitT<float>(s, a, p.grid, p.lds, pass_b, in, out, kern);
}

}  // namespace rdl
