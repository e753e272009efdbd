// The spectral fit of ComponentList::Write (cpp/component_list.cc:105-117)
// for a whole component list at once: the reference calls
// SpectralFitter::Fit once per component on the host; here one lane fits one
// component and returns its terms. Spectra come in channel-major and terms go
// out term-major, so the 64 lanes of a wave read and write consecutive floats.
// The fits themselves are those of the loops and of InterpolateAndStoreModel
// (logpoly.h, unchanged), so the device terms are the host fitter's terms.
//
// Bound: the log-polynomial fit is double-precision Gauss-Newton per lane
// (latency of dependent f64 operations, scratch-resident state: DESIGN.md);
// the polynomial and forced fits are a few f64 operations per value and the
// pass is bound by the copies around it.
#include "rdl_internal.h"

#include "logpoly.h"

namespace rdl {

// lanes per launch: more components go round the grid-stride loops
constexpr unsigned kTermsBlock = 256, kTermsMaxBlocks = 1024;
// the log-polynomial fit keeps few waves per SIMD, so its waves are spread
// over the CUs as single-wave blocks
constexpr unsigned kFitBlock = 64, kFitMaxBlocks = 4096;

// map: n_terms x n_channels doubles, then n_channels fitted flags (in LDS)
__global__ __launch_bounds__(kTermsBlock) void PolynomialTermsKernel(
    const double* map, const uint8_t* fitted, uint32_t n_channels, uint32_t n_terms,
    const float* values, size_t value_stride, size_t n, float* terms, size_t term_stride) {
  extern __shared__ __align__(16) unsigned char lds[];
  double* m = reinterpret_cast<double*>(lds);
  uint8_t* on = lds + size_t(n_terms) * n_channels * sizeof(double);
  for (uint32_t i = threadIdx.x; i < n_terms * n_channels; i += blockDim.x) m[i] = map[i];
  for (uint32_t i = threadIdx.x; i < n_channels; i += blockDim.x) on[i] = fitted[i];
  __syncthreads();
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    // the spectrum is read again for every term (from cache): no per-lane
    // array, so nothing of this kernel lives in scratch
    for (uint32_t t = 0; t < n_terms; ++t) {
      double sum = 0.0;
      for (uint32_t c = 0; c < n_channels; ++c)
        if (on[c]) sum += m[t * n_channels + c] * double(values[size_t(c) * value_stride + i]);
      terms[size_t(t) * term_stride + i] = float(sum);
    }
  }
}

__global__ __launch_bounds__(kFitBlock) void LogPolyTermsKernel(
    rdl_logpoly f, const float* values, size_t value_stride, size_t n, float* terms,
    size_t term_stride) {
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    float v[lp::kMaxCh], t[lp::kMaxTerms];
    for (uint32_t c = 0; c < f.n_channels; ++c) v[c] = values[size_t(c) * value_stride + i];
    lp::Fit(f, v, t);
    for (uint32_t k = 0; k < f.n_terms; ++k) terms[size_t(k) * term_stride + i] = t[k];
  }
}

__global__ __launch_bounds__(kTermsBlock) void ForcedTermsKernel(
    rdl_logpoly f, rdl_forced_terms planes, const uint32_t* x, const uint32_t* y,
    const float* values, size_t value_stride, size_t n, float* terms, size_t term_stride) {
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    float v[lp::kMaxCh], t[lp::kMaxTerms];
    for (uint32_t c = 0; c < f.n_channels; ++c) v[c] = values[size_t(c) * value_stride + i];
    // the launcher checked every (x, y) against the image and the planes
    lp::LoadForcedTerms(planes, f.n_terms, x[i], y[i], t);
    double shape[lp::kMaxCh];
    t[0] = lp::ForcedFit(f, planes.weights, t, v, shape);
    for (uint32_t k = 0; k < f.n_terms; ++k) terms[size_t(k) * term_stride + i] = t[k];
  }
}

}  // namespace rdl

extern "C" int rdl_component_terms(rdl_session* s, uint32_t mode, uint32_t n_channels,
                                   uint32_t n_terms, const double* h_fit,
                                   const uint8_t* h_fitted, const rdl_logpoly* fit,
                                   const rdl_forced_terms* forced, uint32_t width,
                                   uint32_t height, const uint32_t* h_x, const uint32_t* h_y,
                                   const float* d_values, size_t value_stride,
                                   size_t n_components, float* d_terms, size_t term_stride) {
  RDL_ARG_CHECK(s && d_values && d_terms, "NULL argument");
  RDL_ARG_CHECK(mode == RDL_TERMS_POLYNOMIAL || mode == RDL_TERMS_LOGPOLY ||
                    mode == RDL_TERMS_FORCED,
                "component terms: unknown mode");
  if (mode == RDL_TERMS_POLYNOMIAL) {
    RDL_ARG_CHECK(h_fit && h_fitted, "NULL argument");
    RDL_ARG_CHECK(n_channels >= 1 && n_channels <= RDL_MAX_IMAGES,
                  "component terms: channel count out of range");
    RDL_ARG_CHECK(n_terms >= 1 && n_terms <= RDL_MAX_IMAGES,
                  "component terms: term count out of range");
  } else {
    RDL_ARG_CHECK(fit, "NULL argument");
    RDL_ARG_CHECK(n_channels >= 1 && n_channels <= RDL_LOGPOLY_MAX_CHANNELS,
                  "component terms: channel count out of range");
    RDL_ARG_CHECK(n_terms >= 1 && n_terms <= RDL_LOGPOLY_MAX_TERMS,
                  "component terms: term count out of range");
    RDL_ARG_CHECK(fit->n_channels == n_channels && fit->n_terms == n_terms,
                  "component terms: the counts differ from the fit's");
  }
  RDL_ARG_CHECK(n_channels == 1 || value_stride >= n_components, "value planes overlap");
  RDL_ARG_CHECK(n_terms == 1 || term_stride >= n_components, "term planes overlap");
  if (mode == RDL_TERMS_FORCED) {
    RDL_ARG_CHECK(forced && h_x && h_y, "NULL argument");
    RDL_ARG_CHECK(rdl::lp::ForcedTermsCover(*forced, n_terms, width, height),
                  "forced-term planes do not cover the image");
    for (size_t i = 0; i != n_components; ++i)
      RDL_ARG_CHECK(h_x[i] < width && h_y[i] < height,
                    "component terms: a component lies outside the image");
  }
  if (n_components == 0) return RDL_OK;
  const size_t n = n_components;
  const double bytes = double(n) * 4.0 * double(n_channels + n_terms);
  if (mode == RDL_TERMS_POLYNOMIAL) {
    const size_t map_bytes = size_t(n_terms) * n_channels * sizeof(double);
    RDL_TRY(s->EnsureScratch(s->kernel, map_bytes + n_channels));
    char* d_map = static_cast<char*>(s->kernel.ptr);
    RDL_HIP_CHECK(hipMemcpyAsync(d_map, h_fit, map_bytes, hipMemcpyHostToDevice, s->stream));
    RDL_HIP_CHECK(hipMemcpyAsync(d_map + map_bytes, h_fitted, n_channels,
                                 hipMemcpyHostToDevice, s->stream));
    const unsigned grid = unsigned(
        std::min<size_t>((n + rdl::kTermsBlock - 1) / rdl::kTermsBlock, rdl::kTermsMaxBlocks));
    rdl::ScopedTiming t(s, "component_terms", bytes);
    // at most 64 x 64 doubles + 64 flags: under the 64 KiB a launch may ask for
    rdl::PolynomialTermsKernel<<<grid, rdl::kTermsBlock, map_bytes + n_channels, s->stream>>>(
        reinterpret_cast<const double*>(d_map),
        reinterpret_cast<const uint8_t*>(d_map + map_bytes), n_channels, n_terms, d_values,
        value_stride, n, d_terms, term_stride);
  } else if (mode == RDL_TERMS_LOGPOLY) {
    const unsigned grid = unsigned(
        std::min<size_t>((n + rdl::kFitBlock - 1) / rdl::kFitBlock, rdl::kFitMaxBlocks));
    rdl::ScopedTiming t(s, "component_terms", bytes);
    rdl::LogPolyTermsKernel<<<grid, rdl::kFitBlock, 0, s->stream>>>(*fit, d_values, value_stride,
                                                                   n, d_terms, term_stride);
  } else {
    // the positions go through the session's grow-only upload scratch, which
    // otherwise holds small host-provided kernels: 8 bytes per component
    // (7.5 MB at 937,217) that stay with the session until it is destroyed
    RDL_TRY(s->EnsureScratch(s->kernel, 2 * n * sizeof(uint32_t)));
    uint32_t* d_x = static_cast<uint32_t*>(s->kernel.ptr);
    uint32_t* d_y = d_x + n;
    RDL_HIP_CHECK(hipMemcpyAsync(d_x, h_x, n * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 s->stream));
    RDL_HIP_CHECK(hipMemcpyAsync(d_y, h_y, n * sizeof(uint32_t), hipMemcpyHostToDevice,
                                 s->stream));
    const unsigned grid = unsigned(
        std::min<size_t>((n + rdl::kTermsBlock - 1) / rdl::kTermsBlock, rdl::kTermsMaxBlocks));
    rdl::ScopedTiming t(s, "component_terms", bytes + double(n) * 4.0 * double(n_terms + 1));
    rdl::ForcedTermsKernel<<<grid, rdl::kTermsBlock, 0, s->stream>>>(
        *fit, *forced, d_x, d_y, d_values, value_stride, n, d_terms, term_stride);
  }
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}
