#include "deconvolution_algorithm.h"

#include <atomic>
#include <stdexcept>
#include <string>

#include "logpoly.h"
#include "python_deconvolution_factory.h"

namespace radler::algorithms {

namespace {
std::atomic<PythonDeconvolutionFactory> python_factory{nullptr};
}

void SetPythonDeconvolutionFactory(PythonDeconvolutionFactory factory) {
  python_factory.store(factory);
}

std::unique_ptr<DeconvolutionAlgorithm> MakePythonDeconvolution(
    const std::string& filename) {
  const PythonDeconvolutionFactory factory = python_factory.load();
  if (!factory)
    throw std::runtime_error(
        "Python deconvolution needs the radler Python module loaded in the process: "
        "the module hosts the algorithm, and this library embeds no interpreter");
  return factory(filename);
}

void DeconvolutionAlgorithm::SetSpectrallyForcedImages(
    std::vector<std::vector<float>> planes, size_t width) {
  if (!has_forced_)
    throw std::runtime_error(
        "SetSpectrallyForcedImages: the spectral fitter is not in forced-terms mode");
  const uint32_t n_terms = forced_.fit.n_terms;
  if (planes.size() + 1 != n_terms)
    throw std::runtime_error("SetSpectrallyForcedImages: " + std::to_string(planes.size()) +
                             " term planes given, a fit of " + std::to_string(n_terms) +
                             " terms needs " + std::to_string(n_terms - 1));
  auto images = std::make_shared<ForcedTermImages>();
  images->n_planes = planes.size();
  images->width = width;
  for (const std::vector<float>& p : planes) {
    if (width == 0 || p.empty() || p.size() != planes.front().size() || p.size() % width != 0)
      throw std::runtime_error(
          "SetSpectrallyForcedImages: the term planes must be non-empty, of equal size and "
          "made of rows of the given width");
    images->height = p.size() / width;
    images->data.insert(images->data.end(), p.begin(), p.end());
  }
  SetSpectrallyForcedImages(std::move(images), 0, 0);
}

const rdl_logpoly* DeconvolutionAlgorithm::DeviceFit(gpu::Session& s, size_t width,
                                                     size_t height) {
  if (!has_forced_) return LogPolyFit();
  const rdl_logpoly& fit = forced_.fit;
  rdl_forced_terms& terms = forced_.terms;
  forced_.fit.flags = RDL_LOGPOLY_FORCED;
  terms.d_planes = nullptr;
  terms.plane_stride = 0;
  terms.pitch = terms.rows = terms.x0 = terms.y0 = 0;
  if (fit.n_terms <= 1) return &forced_.fit;
  if (!forced_images_)
    throw std::runtime_error(
        "Forced-term spectral fitting needs term images (SetSpectrallyForcedImages)");
  const ForcedTermImages& im = *forced_images_;
  if (im.n_planes + 1 != fit.n_terms || forced_x0_ + width > im.width ||
      forced_y0_ + height > im.height || im.data.size() != im.n_planes * im.width * im.height)
    throw std::runtime_error(
        "The forced spectral-term images do not cover the deconvolved image");
  if (!forced_device_ || forced_device_session_ != &s) {
    forced_device_ = std::make_shared<gpu::Buffer>(s, im.data.size() * sizeof(float));
    s.H2D(forced_device_->Ptr(), im.data.data(), im.data.size() * sizeof(float));
    forced_device_session_ = &s;
  }
  terms.d_planes = forced_device_->F();
  terms.plane_stride = im.width * im.height;
  terms.pitch = uint32_t(im.width);
  terms.rows = uint32_t(im.height);
  terms.x0 = uint32_t(forced_x0_);
  terms.y0 = uint32_t(forced_y0_);
  return &forced_.fit;
}

void DeconvolutionAlgorithm::RejectForcedTermsForOptimization() const {
  if (has_forced_)
    throw std::runtime_error(
        "Component optimization cannot be combined with forced-term spectral fitting");
}

const uint8_t* DeconvolutionAlgorithm::DeviceCleanMask(gpu::Session& s,
                                                       size_t width,
                                                       size_t height) {
  if (!settings_.clean_mask) return nullptr;
  const size_t n = width * height;
  if (!mask_buffer_ || mask_buffer_->Bytes() < n || mask_session_ != &s) {
    mask_buffer_ = std::make_shared<gpu::Buffer>(s, n);
    mask_session_ = &s;
  }
  // bool is one byte holding 0/1: upload as uint8
  s.H2D(mask_buffer_->Ptr(), settings_.clean_mask, n);
  return static_cast<const uint8_t*>(mask_buffer_->Ptr());
}

void DeconvolutionAlgorithm::PerformSpectralFit(float* values, size_t x,
                                                size_t y) const {
  if (!spectral_fitter_) return;
  if (has_forced_) {
    // the terms of the pixel inside the full-image planes (the shared fitter
    // holds no planes: each subimage algorithm has its own origin)
    const rdl_logpoly& fit = forced_.fit;
    float terms[RDL_LOGPOLY_MAX_TERMS] = {};
    if (fit.n_terms > 1) {
      if (!forced_images_)
        throw std::runtime_error(
            "Forced-term spectral fitting needs term images (SetSpectrallyForcedImages)");
      const ForcedTermImages& im = *forced_images_;
      const size_t px = x + forced_x0_, py = y + forced_y0_;
      if (px >= im.width || py >= im.height || im.n_planes + 1 != fit.n_terms)
        throw std::runtime_error(
            "The forced spectral-term images do not cover the deconvolved image");
      for (size_t k = 1; k != fit.n_terms; ++k)
        terms[k] = im.data[((k - 1) * im.height + py) * im.width + px];
    }
    rdl::lp::PerformForcedFit(fit, forced_.terms.weights, terms, uint32_t(n_polarizations_),
                              values);
    return;
  }
  const size_t n = spectral_fitter_->Frequencies().size();
  std::vector<float> channel(n), scratch;
  for (size_t p = 0; p != n_polarizations_; ++p) {
    for (size_t ch = 0; ch != n; ++ch) channel[ch] = values[ch * n_polarizations_ + p];
    spectral_fitter_->FitAndEvaluate(channel.data(), x, y, scratch);
    for (size_t ch = 0; ch != n; ++ch) values[ch * n_polarizations_ + p] = channel[ch];
  }
}

const float* DeconvolutionAlgorithm::DeviceSpectralMap(gpu::Session& s,
                                                       size_t n_images) {
  if (!spectral_fitter_) return nullptr;
  if (spectral_map_images_ != n_images || spectral_map_session_ != &s) {
    spectral_map_images_ = n_images;
    spectral_map_session_ = &s;
    spectral_map_.reset();
    const std::vector<float> g = ComponentFitMatrix(*spectral_fitter_, n_polarizations_);
    spectral_map_identity_ = g.empty();
    if (!g.empty()) {
      if (g.size() != n_images * n_images)
        throw std::runtime_error(
            "Spectral fitting: the image set does not match the fitter's "
            "channels");
      spectral_map_ = std::make_shared<gpu::Buffer>(s, g.size() * sizeof(float));
      s.H2D(spectral_map_->Ptr(), g.data(), g.size() * sizeof(float));
    }
  }
  return spectral_map_identity_ ? nullptr : spectral_map_->F();
}

const float* DeconvolutionAlgorithm::DeviceRmsFactor(gpu::Session& s, size_t width,
                                                     size_t height) {
  if (!rms_factor_) return nullptr;
  const size_t n = width * height;
  if (rms_factor_->size() != n)
    throw std::runtime_error("RMS factor image does not match the image size");
  if (!rms_device_ || rms_device_session_ != &s) {
    rms_device_ = std::make_shared<gpu::Buffer>(s, n * sizeof(float));
    s.H2D(rms_device_->Ptr(), rms_factor_->data(), n * sizeof(float));
    rms_device_session_ = &s;
  }
  return rms_device_->F();
}

const float* DeconvolutionAlgorithm::RmsWeighted(gpu::Session& s, const float* d_image,
                                                 float* d_scratch, size_t width,
                                                 size_t height) {
  const float* rms = DeviceRmsFactor(s, width, height);
  if (!rms) return d_image;
  gpu::Check(rdl_multiply(s.Handle(), d_scratch, d_image, rms, width * height),
             "rdl_multiply");
  return d_scratch;
}

}  // namespace radler::algorithms
