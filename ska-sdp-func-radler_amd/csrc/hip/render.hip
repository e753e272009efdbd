// A component list back into images: the inverse of component_terms.hip.
// rdl_render_components evaluates every component's spectral terms at the
// requested outputs (or takes its values as they are) and stores the fluxes
// as delta planes, one lane per component; rdl_spectrum_multiply_add sums the
// scales' image x kernel spectra so that a model plane costs one inverse
// transform (ComponentList::Render, csrc/host/component_list.cc).
//
// Bound: both kernels move memory. The render reads n_in coalesced floats and
// scatters n_out floats per component (a cache line per store at worst); the
// multiply-add streams 32 bytes per complex element.
#include "rdl_internal.h"

#include <algorithm>

#include "logpoly.h"

namespace rdl {

// lanes per launch (RDL_RENDER_LANES): more components go round the
// grid-stride loop
constexpr unsigned kRenderBlock = 256, kRenderMaxBlocks = 1024;
static_assert(kRenderBlock * kRenderMaxBlocks == RDL_RENDER_LANES, "rdl_hip.h states the lanes");

struct RenderOutputs {
  double at[RDL_MAX_IMAGES];
};

// the launcher checked every (x, y) against width x height and against each
// other, so every store below lands inside its plane and on a pixel of its own
__global__ __launch_bounds__(kRenderBlock) void RenderComponentsKernel(
    uint32_t mode, uint32_t n_in, const float* in, size_t in_stride, size_t n,
    const uint32_t* x, const uint32_t* y, uint32_t width, RenderOutputs out, uint32_t n_out,
    float* planes, size_t plane_stride) {
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    float* pixel = planes + size_t(y[i]) * width + x[i];
    if (mode == RDL_RENDER_VALUES) {
      for (uint32_t g = 0; g < n_out; ++g)
        pixel[size_t(g) * plane_stride] = in[size_t(g) * in_stride + i];
    } else if (mode == RDL_TERMS_POLYNOMIAL) {
      // the terms are read again for every output (from cache): no per-lane
      // array of RDL_MAX_IMAGES floats
      for (uint32_t g = 0; g < n_out; ++g) {
        const float at = float(out.at[g]);
        float value = in[i], power = 1.0f;
        for (uint32_t k = 1; k < n_in; ++k) {
          power *= at;
          value += power * in[size_t(k) * in_stride + i];
        }
        pixel[size_t(g) * plane_stride] = value;
      }
    } else {
      float t[lp::kMaxTerms];
      for (uint32_t k = 0; k < n_in; ++k) t[k] = in[size_t(k) * in_stride + i];
      for (uint32_t g = 0; g < n_out; ++g)
        pixel[size_t(g) * plane_stride] = lp::Evaluate(t, int(n_in), out.at[g]);
    }
  }
}

__global__ __launch_bounds__(256) void SpectrumMultiplyAdd(float2* acc, const float2* a,
                                                           const float2* b, size_t n,
                                                           float scale) {
  for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n;
       i += size_t(gridDim.x) * blockDim.x) {
    const float2 x = a[i], y = b[i];
    float2 r = acc[i];
    r.x += (x.x * y.x - x.y * y.y) * scale;
    r.y += (x.x * y.y + x.y * y.x) * scale;
    acc[i] = r;
  }
}

}  // namespace rdl

extern "C" int rdl_render_components(rdl_session* s, uint32_t mode, uint32_t n_in,
                                     const float* d_in, size_t in_stride, size_t n_components,
                                     const uint32_t* h_x, const uint32_t* h_y, uint32_t width,
                                     uint32_t height, const double* h_out, uint32_t n_out,
                                     float* d_planes, size_t plane_stride) {
  RDL_ARG_CHECK(s && d_planes, "NULL argument");
  RDL_ARG_CHECK(mode == RDL_TERMS_POLYNOMIAL || mode == RDL_TERMS_LOGPOLY ||
                    mode == RDL_TERMS_FORCED || mode == RDL_RENDER_VALUES,
                "render components: unknown mode");
  RDL_ARG_CHECK(n_in >= 1 && n_in <= RDL_MAX_IMAGES,
                "render components: input row count out of range");
  RDL_ARG_CHECK(n_out >= 1 && n_out <= RDL_MAX_IMAGES,
                "render components: output count out of range");
  if (mode == RDL_RENDER_VALUES) {
    RDL_ARG_CHECK(n_out == n_in, "render components: values give one plane per row");
  } else {
    RDL_ARG_CHECK(h_out, "NULL argument");
    RDL_ARG_CHECK(mode == RDL_TERMS_POLYNOMIAL || n_in <= RDL_LOGPOLY_MAX_TERMS,
                  "render components: term count out of range");
  }
  RDL_ARG_CHECK(width > 0 && height > 0, "render components: empty image");
  const size_t plane = size_t(width) * height;
  RDL_ARG_CHECK(n_out == 1 || plane_stride >= plane, "render components: planes overlap");
  RDL_ARG_CHECK(n_components <= plane, "render components: more components than pixels");
  RDL_ARG_CHECK(n_in == 1 || in_stride >= n_components, "render components: input rows overlap");
  if (n_components != 0) {
    RDL_ARG_CHECK(d_in && h_x && h_y, "NULL argument");
    std::vector<uint64_t> pixels(n_components);
    for (size_t i = 0; i != n_components; ++i) {
      RDL_ARG_CHECK(h_x[i] < width && h_y[i] < height,
                    "render components: a component lies outside the image");
      pixels[i] = uint64_t(h_y[i]) * width + h_x[i];
    }
    std::sort(pixels.begin(), pixels.end());
    RDL_ARG_CHECK(std::adjacent_find(pixels.begin(), pixels.end()) == pixels.end(),
                  "render components: two components share a position");
  }
  const size_t n = n_components;
  if (n_out == 1 || plane_stride == plane) {
    RDL_HIP_CHECK(hipMemsetAsync(d_planes, 0, size_t(n_out) * plane * sizeof(float), s->stream));
  } else {
    for (uint32_t g = 0; g != n_out; ++g)
      RDL_HIP_CHECK(hipMemsetAsync(d_planes + size_t(g) * plane_stride, 0,
                                   plane * sizeof(float), s->stream));
  }
  if (n == 0) return RDL_OK;
  // the positions go through the session's grow-only upload scratch, as the
  // forced fit's do (component_terms.hip): 8 bytes per component
  RDL_TRY(s->EnsureScratch(s->kernel, 2 * n * sizeof(uint32_t)));
  uint32_t* d_x = static_cast<uint32_t*>(s->kernel.ptr);
  uint32_t* d_y = d_x + n;
  RDL_HIP_CHECK(hipMemcpyAsync(d_x, h_x, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  RDL_HIP_CHECK(hipMemcpyAsync(d_y, h_y, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
  rdl::RenderOutputs out{};
  for (uint32_t g = 0; h_out && g != n_out; ++g) out.at[g] = h_out[g];
  const unsigned grid = unsigned(
      std::min<size_t>((n + rdl::kRenderBlock - 1) / rdl::kRenderBlock, rdl::kRenderMaxBlocks));
  rdl::ScopedTiming t(s, "render_components", double(n) * 4.0 * double(n_in + n_out + 2));
  rdl::RenderComponentsKernel<<<grid, rdl::kRenderBlock, 0, s->stream>>>(
      mode, n_in, d_in, in_stride, n, d_x, d_y, width, out, n_out, d_planes, plane_stride);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

extern "C" int rdl_spectrum_multiply_add(rdl_session* s, void* d_acc, const void* d_a,
                                         const void* d_b, size_t n_complex, float scale) {
  RDL_ARG_CHECK(s && d_acc && d_a && d_b, "NULL argument");
  if (n_complex == 0) return RDL_OK;
  const unsigned grid = unsigned(std::min<size_t>((n_complex + 255) / 256, size_t(1) << 16));
  rdl::ScopedTiming t(s, "spectrum_multiply_add", double(n_complex) * 32.0);
  rdl::SpectrumMultiplyAdd<<<grid, 256, 0, s->stream>>>(
      static_cast<float2*>(d_acc), static_cast<const float2*>(d_a),
      static_cast<const float2*>(d_b), n_complex, scale);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}
