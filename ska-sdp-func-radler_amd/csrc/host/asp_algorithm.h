// radler::algorithms::AspAlgorithm on the device (reference:
// cpp/algorithms/asp_algorithm.{h,cc}): adaptive scale pixel deconvolution.
// Every minor iteration searches all scales as multiscale clean does, fits an
// elliptical Gaussian to the integrated residual at the winning scale's peak,
// deconvolves it by the fitted PSF ellipse and removes that Gaussian. The
// images stay in HBM; the host sees the scales' peaks, the 28 sums of each
// Levenberg-Marquardt step and the component's per-image values.
//
// Composed from the engine's parts rather than lifted out of
// MultiScaleAlgorithm: its own MultiScaleTransforms, the fused multi-scale
// peak searches, the padded float64 residual correction with one padded PSF
// spectrum per PSF and major iteration, rdl_subtract_psf, and the three
// primitives of csrc/hip/asp.hip.
#pragma once

#include <map>
#include <memory>
#include <vector>

#include "deconvolution_algorithm.h"
#include "gaussian_fit.h"
#include "multiscale_algorithm.h"
#include "multiscale_transforms.h"

namespace radler::algorithms {

class AspAlgorithm final : public DeconvolutionAlgorithm {
 public:
  AspAlgorithm(const Settings::Multiscale& settings, double beam_size, double pixel_scale_x,
               double pixel_scale_y);
  /// Clones share the settings and the scales, not the device state.
  AspAlgorithm(const AspAlgorithm& other);

  std::unique_ptr<DeconvolutionAlgorithm> Clone() const final {
    return std::make_unique<AspAlgorithm>(*this);
  }

  DeconvolutionResult ExecuteMajorIteration(ImageSet& data_image, ImageSet& model_image,
                                            const gpu::Planes& psf_images) final;

  size_t ScaleCount() const { return scale_infos_.size(); }
  float ScaleSize(size_t scale_index) const { return scale_infos_[scale_index].scale; }

 private:
  using ScaleInfo = MultiScaleAlgorithm::ScaleInfo;

  /// asp_algorithm.cc:373-458: the linear integrated residual into
  /// d_integrated, then every scale's peak (scale 0 directly, the others
  /// through the multi-scale transforms), collected with one read.
  void FindScaleConvolvedMaxima(const ImageSet& image_set, float* d_integrated);
  const float* PeakSearchInput(const float* d_image);
  float Normalized(float value, size_t x, size_t y) const;
  void DeconvolvePointSource(size_t x, size_t y, ImageSet& data_image, ImageSet& model_image,
                             const gpu::Planes& psf_images);
  void DeconvolveGaussian(const ScaleInfo& peak_scale, ImageSet& data_image,
                          ImageSet& model_image, const gpu::Planes& psf_images,
                          const float* d_integrated,
                          const schaapcommon::math::Ellipse& psf_parameters);
  /// d_residual -= Trim(Untrim(d_component) (x) PSF) at the padded size, as
  /// SubMinorLoop::CorrectResidualDirtyWithSpectrum does for its model.
  void CorrectResidual(float* d_residual, const float* d_component, size_t psf_index,
                       const gpu::Planes& psf_images);

  const Settings::Multiscale& settings_;
  double beam_size_in_pixels_;
  std::vector<ScaleInfo> scale_infos_;

  // per-major-iteration device state
  gpu::Session* session_ = nullptr;
  size_t width_ = 0, height_ = 0, padded_width_ = 0, padded_height_ = 0;
  std::unique_ptr<multiscale::MultiScaleTransforms> transforms_;
  const uint8_t* d_mask_ = nullptr;
  std::shared_ptr<gpu::Buffer> scratch_;      // W x H: a scale's image, a component
  std::shared_ptr<gpu::Buffer> rms_scratch_;  // W x H: image x RMS factor
  std::shared_ptr<gpu::Buffer> spectrum_, spectrum_work_;
  std::vector<std::shared_ptr<gpu::Buffer>> scale_u_;  // the fused path's inner inverses
  std::shared_ptr<gpu::Buffer> padded_, padded_f64_;   // rocFFT correction planes
  // the padded PSF spectra of this major iteration, made when first used
  std::map<size_t, std::shared_ptr<gpu::Buffer>> psf_spectra_;
};

}  // namespace radler::algorithms
