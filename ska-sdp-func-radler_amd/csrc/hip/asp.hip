// The device primitives of the adaptive-scale-pixel algorithm
// (cpp/algorithms/asp_algorithm.cc): the normal-equation sums of an
// elliptical Gaussian fit, the Gaussian renderer, and the Gaussian-weighted
// value of a plane at one pixel. All three share one Gaussian (rdl_hip.h,
// "adaptive scale pixel") evaluated in double.
//
// The reductions are deterministic: every thread accumulates its pixels in
// index order, a wave64 butterfly and a fixed-order sum over the block's four
// waves give one partial row per block in a device slab, and a second launch
// sums the slab's rows in a fixed order. No floating-point atomics; the grids
// depend on the box size only.
#include <algorithm>
#include <cmath>

#include "rdl_internal.h"

namespace rdl {
namespace {

constexpr unsigned kThreads = 256;
constexpr unsigned kWaves = kThreads / 64;
constexpr unsigned kPixelsPerBlock = 1024;
constexpr unsigned kMaxFitBlocks = 1024;
constexpr unsigned kMaxValueChunks = 256;
constexpr int kFitSums = RDL_GAUSSIAN_FIT_SUMS;
// FWHM -> sigma: 1 / (2 sqrt(2 ln 2))
constexpr double kFwhmToSigma = 0.42466090014400953;
// regions of the session's result buffer (rdl_internal.h kMapped*)
constexpr size_t kMappedGaussianFit = 1024;     // 28 doubles
constexpr size_t kMappedGaussianValues = 2048;  // RDL_GAUSSIAN_MAX_PLANES doubles

struct Shape {
  double cs, sn;              // cos, sin of the position angle
  double inv_maj2, inv_min2;  // 1 / sigma^2
  double norm;                // 1 / (2 pi sigma_maj sigma_min)
  double sigma_maj;
};

Shape MakeShape(double fwhm_major, double fwhm_minor, double pa) {
  Shape e;
  const double sm = fwhm_major * kFwhmToSigma, sn = fwhm_minor * kFwhmToSigma;
  e.cs = std::cos(pa);
  e.sn = std::sin(pa);
  e.inv_maj2 = 1.0 / (sm * sm);
  e.inv_min2 = 1.0 / (sn * sn);
  e.norm = 1.0 / (2.0 * M_PI * sm * sn);
  e.sigma_maj = sm;
  return e;
}

// the half-side of the 6 sigma box, never more than the plane needs
uint32_t HalfSide(const Shape& e, uint32_t width, uint32_t height) {
  const double h = std::ceil(6.0 * e.sigma_maj);
  const double cap = double(std::max(width, height));
  return uint32_t(std::min(h, cap));
}

// acc[k] summed over the block into row[k] (threads k < N store it)
template <int N>
__device__ __forceinline__ void BlockSums(double (&acc)[N], double* lds, double* row) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    acc[k] = v;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) lds[wave * N + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double v = lds[threadIdx.x];
    for (unsigned w = 1; w < kWaves; ++w) v += lds[w * N + threadIdx.x];
    row[threadIdx.x] = v;
  }
}

struct FitArgs {
  const float* image;
  uint32_t width;
  uint32_t bx, by, bw, bh;
  double amplitude, x0, y0;
  double cs, sn, inv_maj2, inv_min2, inv_fwhm_maj, inv_fwhm_min;
  double* slab;
};

__global__ __launch_bounds__(256) void GaussianFitSumsKernel(FitArgs p) {
  __shared__ double lds[kWaves * kFitSums];
  double acc[kFitSums];
#pragma unroll
  for (int k = 0; k < kFitSums; ++k) acc[k] = 0.0;
  const size_t n = size_t(p.bw) * p.bh;
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    const uint32_t x = p.bx + uint32_t(i % p.bw), y = p.by + uint32_t(i / p.bw);
    const double dx = double(x) - p.x0, dy = double(y) - p.y0;
    const double u = dx * p.cs + dy * p.sn;
    const double v = dy * p.cs - dx * p.sn;
    const double um = u * p.inv_maj2, vm = v * p.inv_min2;
    const double e = exp(-0.5 * (u * um + v * vm));
    const double ae = p.amplitude * e;
    const double r = double(p.image[size_t(y) * p.width + x]) - ae;
    double j[6];
    j[0] = e;
    j[1] = ae * (um * p.cs - vm * p.sn);
    j[2] = ae * (um * p.sn + vm * p.cs);
    j[3] = ae * (u * um * p.inv_fwhm_maj);
    j[4] = ae * (v * vm * p.inv_fwhm_min);
    j[5] = ae * (u * v * (p.inv_min2 - p.inv_maj2));
    int t = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) acc[t++] += j[a] * j[b];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += j[a] * r;
    acc[27] += r * r;
  }
  BlockSums<kFitSums>(acc, lds, p.slab + size_t(blockIdx.x) * kFitSums);
}

// out[c] = the sum of slab[r][c] over the rows, c < n_cols <= 32: eight
// interleaved row sequences per column, each in row order, then the eight in
// order. One block.
__global__ __launch_bounds__(256) void SlabSumKernel(const double* slab, uint32_t n_rows,
                                                     uint32_t n_cols, double* out) {
  __shared__ double lds[8 * 32];
  const uint32_t col = threadIdx.x & 31, seg = threadIdx.x >> 5;
  double v = 0.0;
  if (col < n_cols)
    for (uint32_t r = seg; r < n_rows; r += 8) v += slab[size_t(r) * n_cols + col];
  lds[seg * 32 + col] = v;
  __syncthreads();
  if (threadIdx.x < n_cols) {
    double sum = lds[threadIdx.x];
    for (uint32_t s = 1; s < 8; ++s) sum += lds[s * 32 + threadIdx.x];
    out[threadIdx.x] = sum;
  }
}

struct DrawArgs {
  float* plane;
  uint32_t width;
  uint32_t bx, by, bw, bh;
  double x0, y0, scale;  // scale = flux / (2 pi sigma_maj sigma_min)
  double cs, sn, inv_maj2, inv_min2;
};

__global__ __launch_bounds__(256) void DrawGaussianKernel(DrawArgs p) {
  const size_t n = size_t(p.bw) * p.bh;
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    const uint32_t x = p.bx + uint32_t(i % p.bw), y = p.by + uint32_t(i / p.bw);
    const double dx = double(x) - p.x0, dy = double(y) - p.y0;
    const double u = dx * p.cs + dy * p.sn;
    const double v = dy * p.cs - dx * p.sn;
    const double e = exp(-0.5 * (u * u * p.inv_maj2 + v * v * p.inv_min2));
    const size_t idx = size_t(y) * p.width + x;
    p.plane[idx] += float(p.scale * e);
  }
}

struct ValueArgs {
  const float* planes;
  size_t stride;
  uint32_t width, height, half;
  double cs, sn, inv_maj2, inv_min2, norm;
  double* slab;
  uint32_t cx[RDL_GAUSSIAN_MAX_PLANES], cy[RDL_GAUSSIAN_MAX_PLANES];
};

// block (chunk, plane): the chunk's share of the plane's clipped box
__global__ __launch_bounds__(256) void GaussianValuesKernel(ValueArgs p) {
  __shared__ double lds[kWaves];
  const uint32_t plane = blockIdx.y;
  const uint32_t cx = p.cx[plane], cy = p.cy[plane];
  const uint32_t x_lo = cx > p.half ? cx - p.half : 0u;
  const uint32_t y_lo = cy > p.half ? cy - p.half : 0u;
  const uint32_t x_hi = min(p.width - 1u, cx + p.half);  // cx < width, half <= max side
  const uint32_t y_hi = min(p.height - 1u, cy + p.half);
  const uint32_t bw = x_hi - x_lo + 1u, bh = y_hi - y_lo + 1u;
  const size_t n = size_t(bw) * bh;
  const float* image = p.planes + size_t(plane) * p.stride;
  double acc[1] = {0.0};
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    const uint32_t x = x_lo + uint32_t(i % bw), y = y_lo + uint32_t(i / bw);
    const double dx = double(x) - double(cx), dy = double(y) - double(cy);
    const double u = dx * p.cs + dy * p.sn;
    const double v = dy * p.cs - dx * p.sn;
    const double w = p.norm * exp(-0.5 * (u * u * p.inv_maj2 + v * v * p.inv_min2));
    acc[0] += w * double(image[size_t(y) * p.width + x]);
  }
  BlockSums<1>(acc, lds, p.slab + size_t(plane) * gridDim.x + blockIdx.x);
}

// one wave per plane: lane l sums chunks l, l + 64, ... in order
__global__ __launch_bounds__(64) void GaussianValuesFinalKernel(const double* slab,
                                                                uint32_t n_chunks, double* out) {
  const double* row = slab + size_t(blockIdx.x) * n_chunks;
  double v = 0.0;
  for (uint32_t c = threadIdx.x; c < n_chunks; c += 64) v += row[c];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

bool ValidEllipse(double fwhm_major, double fwhm_minor, double pa) {
  return std::isfinite(fwhm_major) && std::isfinite(fwhm_minor) && std::isfinite(pa) &&
         fwhm_major > 0.0 && fwhm_minor > 0.0;
}

}  // namespace
}  // namespace rdl

extern "C" {

int rdl_gaussian_fit_sums(rdl_session* s, const float* d_image, uint32_t width,
                          uint32_t height, uint32_t box_x, uint32_t box_y, uint32_t box_w,
                          uint32_t box_h, const double* params, double* out) {
  RDL_ARG_CHECK(s && d_image && params && out, "NULL argument");
  RDL_ARG_CHECK(box_w >= 1 && box_h >= 1 && box_x < width && box_y < height &&
                    box_w <= width - box_x && box_h <= height - box_y,
                "the box must lie inside the image");
  for (int k = 0; k < 6; ++k) RDL_ARG_CHECK(std::isfinite(params[k]), "non-finite parameter");
  RDL_ARG_CHECK(params[3] > 0.0 && params[4] > 0.0, "FWHM must be positive");
  const rdl::Shape e = rdl::MakeShape(params[3], params[4], params[5]);
  const size_t n = size_t(box_w) * box_h;
  const unsigned grid = unsigned(
      std::min<size_t>((n + rdl::kPixelsPerBlock - 1) / rdl::kPixelsPerBlock, rdl::kMaxFitBlocks));
  RDL_TRY(s->EnsureScratch(s->partials, size_t(rdl::kMaxFitBlocks) * rdl::kFitSums * 8));
  double* slab = static_cast<double*>(s->partials.ptr);
  double* d_out = static_cast<double*>(rdl::MappedResult(s, rdl::kMappedGaussianFit));
  rdl::FitArgs a;
  a.image = d_image;
  a.width = width;
  a.bx = box_x;
  a.by = box_y;
  a.bw = box_w;
  a.bh = box_h;
  a.amplitude = params[0];
  a.x0 = params[1];
  a.y0 = params[2];
  a.cs = e.cs;
  a.sn = e.sn;
  a.inv_maj2 = e.inv_maj2;
  a.inv_min2 = e.inv_min2;
  a.inv_fwhm_maj = 1.0 / params[3];
  a.inv_fwhm_min = 1.0 / params[4];
  a.slab = slab;
  {
    rdl::ScopedTiming t(s, "gaussian_fit", 4.0 * double(n));
    rdl::GaussianFitSumsKernel<<<grid, rdl::kThreads, 0, s->stream>>>(a);
    rdl::SlabSumKernel<<<1, rdl::kThreads, 0, s->stream>>>(slab, grid, rdl::kFitSums, d_out);
    RDL_HIP_CHECK(hipGetLastError());
  }
  const rdl::SmallRead r{out, d_out, rdl::kFitSums * sizeof(double)};
  return rdl::ReadSmall(s, &r, 1);
}

int rdl_draw_gaussian(rdl_session* s, float* d_plane, uint32_t width, uint32_t height,
                      double x0, double y0, double fwhm_major, double fwhm_minor, double pa,
                      double flux) {
  RDL_ARG_CHECK(s && d_plane, "NULL argument");
  RDL_ARG_CHECK(width >= 1 && height >= 1, "empty plane");
  RDL_ARG_CHECK(std::isfinite(x0) && std::isfinite(y0) && std::isfinite(flux),
                "non-finite centre or flux");
  RDL_ARG_CHECK(rdl::ValidEllipse(fwhm_major, fwhm_minor, pa), "bad ellipse");
  const rdl::Shape e = rdl::MakeShape(fwhm_major, fwhm_minor, pa);
  const double half = double(rdl::HalfSide(e, width, height));
  // every pixel within `half` of the centre along both axes, clipped
  const double x_lo = std::max(0.0, std::floor(x0 - half));
  const double x_hi = std::min(double(width - 1), std::ceil(x0 + half));
  const double y_lo = std::max(0.0, std::floor(y0 - half));
  const double y_hi = std::min(double(height - 1), std::ceil(y0 + half));
  if (x_lo > x_hi || y_lo > y_hi) return RDL_OK;  // the box misses the plane
  rdl::DrawArgs a;
  a.plane = d_plane;
  a.width = width;
  a.bx = uint32_t(x_lo);
  a.by = uint32_t(y_lo);
  a.bw = uint32_t(x_hi - x_lo) + 1u;
  a.bh = uint32_t(y_hi - y_lo) + 1u;
  a.x0 = x0;
  a.y0 = y0;
  a.scale = flux * e.norm;
  a.cs = e.cs;
  a.sn = e.sn;
  a.inv_maj2 = e.inv_maj2;
  a.inv_min2 = e.inv_min2;
  const size_t n = size_t(a.bw) * a.bh;
  const unsigned grid =
      unsigned(std::min<size_t>((n + rdl::kThreads - 1) / rdl::kThreads, 8192));
  rdl::ScopedTiming t(s, "gaussian_draw", 8.0 * double(n));
  rdl::DrawGaussianKernel<<<grid, rdl::kThreads, 0, s->stream>>>(a);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_gaussian_weighted_values(rdl_session* s, const float* d_planes, size_t plane_stride,
                                 uint32_t n_planes, uint32_t width, uint32_t height,
                                 const uint32_t* centre_x, const uint32_t* centre_y,
                                 double fwhm_major, double fwhm_minor, double pa, double* out) {
  RDL_ARG_CHECK(s && d_planes && centre_x && centre_y && out, "NULL argument");
  RDL_ARG_CHECK(n_planes >= 1 && n_planes <= RDL_GAUSSIAN_MAX_PLANES, "bad plane count");
  RDL_ARG_CHECK(width >= 1 && height >= 1, "empty plane");
  RDL_ARG_CHECK(n_planes == 1 || plane_stride >= size_t(width) * height,
                "planes overlap");
  RDL_ARG_CHECK(rdl::ValidEllipse(fwhm_major, fwhm_minor, pa), "bad ellipse");
  for (uint32_t i = 0; i < n_planes; ++i)
    RDL_ARG_CHECK(centre_x[i] < width && centre_y[i] < height,
                  "a centre lies outside its plane");
  const rdl::Shape e = rdl::MakeShape(fwhm_major, fwhm_minor, pa);
  rdl::ValueArgs a;
  a.planes = d_planes;
  a.stride = plane_stride;
  a.width = width;
  a.height = height;
  a.half = rdl::HalfSide(e, width, height);
  a.cs = e.cs;
  a.sn = e.sn;
  a.inv_maj2 = e.inv_maj2;
  a.inv_min2 = e.inv_min2;
  a.norm = e.norm;
  for (uint32_t i = 0; i < RDL_GAUSSIAN_MAX_PLANES; ++i) {
    a.cx[i] = i < n_planes ? centre_x[i] : 0u;
    a.cy[i] = i < n_planes ? centre_y[i] : 0u;
  }
  // the chunks follow from the box (clipped to the plane's sides) alone
  const size_t side = 2 * size_t(a.half) + 1;
  const size_t n = std::min<size_t>(side, width) * std::min<size_t>(side, height);
  const unsigned chunks = unsigned(std::min<size_t>(
      (n + rdl::kPixelsPerBlock - 1) / rdl::kPixelsPerBlock, rdl::kMaxValueChunks));
  RDL_TRY(s->EnsureScratch(
      s->partials, size_t(RDL_GAUSSIAN_MAX_PLANES) * rdl::kMaxValueChunks * sizeof(double)));
  a.slab = static_cast<double*>(s->partials.ptr);
  double* d_out = static_cast<double*>(rdl::MappedResult(s, rdl::kMappedGaussianValues));
  {
    rdl::ScopedTiming t(s, "gaussian_weighted", 4.0 * double(n) * n_planes);
    rdl::GaussianValuesKernel<<<dim3(chunks, n_planes), rdl::kThreads, 0, s->stream>>>(a);
    rdl::GaussianValuesFinalKernel<<<n_planes, 64, 0, s->stream>>>(a.slab, chunks, d_out);
    RDL_HIP_CHECK(hipGetLastError());
  }
  const rdl::SmallRead r{out, d_out, n_planes * sizeof(double)};
  return rdl::ReadSmall(s, &r, 1);
}

}  // extern "C"
