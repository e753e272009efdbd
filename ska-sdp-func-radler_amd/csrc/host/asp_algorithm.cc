// AspAlgorithm on the device. Line references are to the reference's
// cpp/algorithms/asp_algorithm.cc unless stated.
#include "asp_algorithm.h"

#include <algorithm>
#include <cmath>
#include <optional>
#include <stdexcept>

#include "fft_sizes.h"
#include "host_profile.h"
#include "logger.h"
#include "scale_search.h"
#include "subminor.h"

namespace radler::algorithms {

using schaapcommon::math::Ellipse;

namespace {
// A deconvolved ellipse narrower than this cannot be sampled on the pixel
// grid (the rendered Gaussian's sum leaves 1): see DeconvolveGaussian.
constexpr double kMinimumFwhm = 1.0;
}  // namespace

AspAlgorithm::AspAlgorithm(const Settings::Multiscale& settings, double beam_size,
                           double pixel_scale_x, double pixel_scale_y)
    : settings_(settings),
      beam_size_in_pixels_(beam_size / std::max(pixel_scale_x, pixel_scale_y)) {
  if (!(beam_size_in_pixels_ > 0.0)) beam_size_in_pixels_ = 1;  // :34
}

AspAlgorithm::AspAlgorithm(const AspAlgorithm& o)
    : DeconvolutionAlgorithm(o),
      settings_(o.settings_),
      beam_size_in_pixels_(o.beam_size_in_pixels_),
      scale_infos_(o.scale_infos_) {}

const float* AspAlgorithm::PeakSearchInput(const float* d_image) {
  if (!RmsFactorImage()) return d_image;
  return RmsWeighted(*session_, d_image, rms_scratch_->F(), width_, height_);
}

float AspAlgorithm::Normalized(float value, size_t x, size_t y) const {
  if (!RmsFactorImage()) return value;
  return value / (*RmsFactorImage())[x + y * width_];
}

void AspAlgorithm::FindScaleConvolvedMaxima(const ImageSet& image_set, float* d_integrated) {
  prof::Section prof_section("asp.find_maxima");
  rdl_session* s = session_->Handle();
  const size_t w = width_, h = height_;
  image_set.GetLinearIntegrated(d_integrated);
  if (scale_infos_.size() > RDL_PEAK_SLOTS)
    throw std::runtime_error("AspAlgorithm: too many scales");
  auto search_input = [&](const float* d_image) { return PeakSearchInput(d_image); };
  std::vector<size_t> pending;  // the scale of each queued search (slot = index)
  std::vector<ConvolvedScale> convolved;
  for (size_t si = 0; si != scale_infos_.size(); ++si) {
    const float scale = scale_infos_[si].scale;
    if (scale == 0.0f) {
      // FindPeakDirect (:412-458): the delta scale is not convolved
      const Borders border = PeakBorders(w, h);
      gpu::Check(rdl_find_peak_enqueue(s, search_input(d_integrated), uint32_t(w), uint32_t(h),
                                       0, uint32_t(h), border.horizontal, border.vertical,
                                       AllowNegativeComponents(), d_mask_, 1,
                                       uint32_t(pending.size())),
                 "rdl_find_peak_enqueue");
      pending.push_back(si);
    } else {
      // every scale is searched, into the one scratch image, inside the one mask
      convolved.push_back({si, scale, scratch_->F(), d_mask_, PeakBorders(w, h, scale)});
    }
  }
  if (!convolved.empty()) {
    ScaleSearch search{*session_, *transforms_, spectrum_->Ptr(),
                       {spectrum_work_->Ptr(), nullptr},  // no lanes
                       scale_u_, AllowNegativeComponents()};
    if (!RmsFactorImage() && transforms_->Fused())
      search.Fused(d_integrated, convolved, false, pending);
    else
      search.ThroughSpectrum(d_integrated, convolved, !RmsFactorImage(), false, pending,
                             search_input);
  }
  CollectPeaks(s, pending, scale_infos_,
               [&](float v, size_t x, size_t y) { return Normalized(v, x, y); });
}

DeconvolutionResult AspAlgorithm::ExecuteMajorIteration(ImageSet& data_image,
                                                        ImageSet& model_image,
                                                        const gpu::Planes& psfs) {
  prof::Section prof_section("asp.execute");
  gpu::Session& session = data_image.Session();
  session_ = &session;
  const size_t width = data_image.Width();
  const size_t height = data_image.Height();
  const size_t npx = width * height;
  width_ = width;
  height_ = height;

  if (StopOnNegativeComponents()) SetAllowNegativeComponents(true);  // :50
  InitializeScales(scale_infos_, beam_size_in_pixels_, std::min(width, height),
                   settings_.shape, settings_.max_scales, settings_.scale_list);
  if (RmsFactorImage() && RmsFactorImage()->size() != npx)  // :56-59
    throw std::runtime_error("Error in RMS factor image dimensions!");
  if (data_image.Size() > RDL_GAUSSIAN_MAX_PLANES)
    throw std::runtime_error("AspAlgorithm: too many images in the set");

  // the correction's padded size: the largest scale's (:64-67)
  padded_width_ = utils::GetConvolutionSize(scale_infos_.back().scale, width,
                                            settings_.convolution_padding);
  padded_height_ = utils::GetConvolutionSize(scale_infos_.back().scale, height,
                                             settings_.convolution_padding);
  if (EnsureTransforms(transforms_, session, width, height, settings_.shape, &scale_infos_))
    scale_u_.clear();
  d_mask_ = DeviceCleanMask(session, width, height);
  scratch_ = std::make_shared<gpu::Buffer>(session, npx * sizeof(float));
  rms_scratch_.reset();
  if (RmsFactorImage())
    rms_scratch_ = std::make_shared<gpu::Buffer>(session, npx * sizeof(float));
  const size_t spectrum_bytes = transforms_->SpectrumBytes();
  spectrum_ = std::make_shared<gpu::Buffer>(session, spectrum_bytes);
  spectrum_work_ = std::make_shared<gpu::Buffer>(session, spectrum_bytes);
  if (!scale_u_.empty() && scale_u_.front()->Bytes() < spectrum_bytes) scale_u_.clear();
  padded_.reset();
  padded_f64_.reset();
  psf_spectra_.clear();
  // the device state of this call goes when it returns
  struct Release {
    AspAlgorithm* a;
    ~Release() {
      a->psf_spectra_.clear();
      a->scratch_.reset();
      a->rms_scratch_.reset();
      a->spectrum_.reset();
      a->spectrum_work_.reset();
      a->padded_.reset();
      a->padded_f64_.reset();
    }
  } release{this};

  gpu::Buffer integrated(session, npx * sizeof(float));
  data_image.GetIntegratedPsf(integrated.F(), psfs);  // :70-71
  const Ellipse psf_parameters = schaapcommon::fitters::Fit2DGaussianCentred(
      session, integrated.F(), width, height, beam_size_in_pixels_);  // :72-73
  log::Debug() << "ASP: PSF ellipse maj=" << psf_parameters.major
               << ", min=" << psf_parameters.minor << ", pa=" << psf_parameters.position_angle
               << '\n';

  // ConvolvePsfs (multiscale_algorithm.cc:29-88) for the integrated PSF: the
  // scales' PSF peaks, bias factors and gains. The per-PSF convolved images
  // of :81-87 feed only the dead work of :138-170 and are not made.
  {
    prof::Section prof_psfs("asp.convolve_psfs");
    const double first_auto_scale_size = beam_size_in_pixels_ * 2.0;
    const size_t n_scales = scale_infos_.size();
    for (size_t si = 0; si != n_scales; ++si) {
      ScaleInfo& e = scale_infos_[si];
      session.D2D(scratch_->F(), integrated.F(), npx * sizeof(float));
      if (e.scale != 0.0f) transforms_->Transform(scratch_->F(), e.scale);
      e.psf_peak = session.ReadFloat(scratch_->F() + width / 2 + (height / 2) * width);
      double exp_term;
      if (e.scale == 0.0f || n_scales < 2)
        exp_term = 0.0;
      else
        exp_term = std::log2(e.scale / first_auto_scale_size);
      e.bias_factor = float(std::pow(settings_.scale_bias, -exp_term));
      e.gain = float(double(MinorLoopGain()) / e.psf_peak);
      e.is_active = true;
      log::Info() << "- Scale " << std::round(e.scale)
                  << ", bias factor=" << std::round(e.bias_factor * 10.0) / 10.0
                  << ", psfpeak=" << e.psf_peak << ", gain=" << e.gain
                  << ", kernel peak=" << e.kernel_peak << '\n';
    }
  }

  FindScaleConvolvedMaxima(data_image, integrated.F());
  DeconvolutionResult result;
  std::optional<size_t> optional_scale = SelectMaximumScale(scale_infos_);
  if (!optional_scale) {
    log::Warn() << "No peak found during ASP cleaning! Aborting deconvolution.\n";
    result.another_iteration_required = false;
    return result;
  }
  size_t scale_with_peak = *optional_scale;

  bool is_final_threshold = false;  // :105-115
  float m_gain_threshold =
      std::fabs(scale_infos_[scale_with_peak].max_unnormalized_image_value *
                scale_infos_[scale_with_peak].bias_factor) *
      (1.0 - MajorLoopGain());
  m_gain_threshold = std::max(m_gain_threshold, MajorIterationThreshold());
  float first_threshold = m_gain_threshold;
  if (Threshold() > first_threshold) {
    first_threshold = Threshold();
    is_final_threshold = true;
  }
  log::Info() << "Starting ASP cleaning. Start peak="
              << scale_infos_[scale_with_peak].max_unnormalized_image_value *
                     scale_infos_[scale_with_peak].bias_factor
              << ", major iteration threshold=" << first_threshold
              << (is_final_threshold ? " (final)\n" : "\n");

  // The minor iteration loop (:132-203). :138-170 convolve the images with the
  // current scale and search them, but :174 overwrites every scale's result
  // before anything reads it: that work is not done here.
  while (IterationNumber() < MaxIterations() &&
         std::fabs(scale_infos_[scale_with_peak].max_unnormalized_image_value *
                   scale_infos_[scale_with_peak].bias_factor) > first_threshold &&
         (!StopOnNegativeComponents() ||
          scale_infos_[scale_with_peak].max_unnormalized_image_value >= 0.0)) {
    SetIterationNumber(IterationNumber() + 1);
    FindScaleConvolvedMaxima(data_image, integrated.F());
    optional_scale = SelectMaximumScale(scale_infos_);
    if (!optional_scale) {
      log::Warn() << "No peak found in main loop of ASP cleaning! Aborting "
                     "deconvolution.\n";
      result.another_iteration_required = false;
      return result;
    }
    scale_with_peak = *optional_scale;
    const ScaleInfo& info = scale_infos_[scale_with_peak];
    log::Info() << "Iteration " << IterationNumber() << ", scale " << std::round(info.scale)
                << " px : " << info.max_unnormalized_image_value * info.bias_factor << " at "
                << info.max_image_value_x << ',' << info.max_image_value_y << '\n';
    if (info.scale == 0.0f)
      DeconvolvePointSource(info.max_image_value_x, info.max_image_value_y, data_image,
                            model_image, psfs);
    else
      DeconvolveGaussian(info, data_image, model_image, psfs, integrated.F(), psf_parameters);
  }

  const bool max_iter_reached = IterationNumber() >= MaxIterations();
  const bool negative_reached =
      StopOnNegativeComponents() &&
      scale_infos_[scale_with_peak].max_unnormalized_image_value < 0.0;
  if (max_iter_reached)
    log::Info() << "ASP finished because maximum number of iterations was reached.\n";
  else if (negative_reached)
    log::Info() << "ASP finished because a negative component was found.\n";
  else if (is_final_threshold)
    log::Info() << "ASP finished because the final threshold was reached.\n";
  else
    log::Info() << "ASP minor loop finished, continuing cleaning after "
                   "inversion/prediction round.\n";
  result.another_iteration_required =
      !max_iter_reached && !is_final_threshold && !negative_reached;
  result.final_peak_value = scale_infos_[scale_with_peak].max_unnormalized_image_value *
                            scale_infos_[scale_with_peak].bias_factor;
  session.Sync();
  return result;
}

void AspAlgorithm::DeconvolvePointSource(size_t x, size_t y, ImageSet& data_image,
                                         ImageSet& model_image,
                                         const gpu::Planes& psfs) {  // :231-254
  prof::Section prof_section("asp.point_source");
  rdl_session* s = session_->Handle();
  const size_t index = x + y * width_;
  std::vector<float> values(data_image.Size());
  for (size_t i = 0; i != data_image.Size(); ++i)
    values[i] = session_->ReadFloat(data_image.Data(i) + index);
  PerformSpectralFit(values.data(), x, y);
  const float unit = 1.0f;
  for (size_t i = 0; i != data_image.Size(); ++i) {
    values[i] *= MinorLoopGain();
    // model[index] += value (fma(1, v, m) == m + v)
    gpu::Check(rdl_add_shape_component(s, model_image.Data(i), uint32_t(width_),
                                       uint32_t(height_), &unit, 1, uint32_t(x), uint32_t(y),
                                       values[i]),
               "rdl_add_shape_component");
    gpu::Check(rdl_subtract_psf(s, data_image.Data(i), psfs.Plane(data_image.PsfIndex(i)),
                                uint32_t(width_), uint32_t(height_), uint32_t(x), uint32_t(y),
                                values[i]),
               "rdl_subtract_psf");
  }
}

void AspAlgorithm::DeconvolveGaussian(const ScaleInfo& peak_scale, ImageSet& data_image,
                                      ImageSet& model_image, const gpu::Planes& psfs,
                                      const float* d_integrated,
                                      const Ellipse& psf_parameters) {  // :256-371
  rdl_session* s = session_->Handle();
  const size_t width = width_, height = height_;
  double fit_a = peak_scale.max_unnormalized_image_value * peak_scale.bias_factor;
  double fit_x = double(peak_scale.max_image_value_x);
  double fit_y = double(peak_scale.max_image_value_y);
  Ellipse gaussian{peak_scale.scale, peak_scale.scale, 0.0};
  {
    // d_integrated holds the linear integrated residual of this iteration's
    // searches (FindScaleConvolvedMaxima)
    prof::Section prof_fit("asp.fit");
    schaapcommon::fitters::Fit2DGaussianFull(*session_, d_integrated, width, height, fit_a,
                                             fit_x, fit_y, gaussian.major, gaussian.minor,
                                             gaussian.position_angle);
  }
  log::Info() << "x=" << fit_x << ", y=" << fit_y << ", a=" << fit_a
              << ", maj=" << gaussian.major << ", min=" << gaussian.minor
              << ", pa=" << gaussian.position_angle << '\n';
  if (!std::isfinite(fit_x) || !std::isfinite(fit_y)) {
    fit_x = double(peak_scale.max_image_value_x);
    fit_y = double(peak_scale.max_image_value_y);
  }
  // :274-275 pass std::clamp its arguments in the wrong order (value 0 clamped
  // to [width - 1, round(fit_x)]); built here is the evident intent
  const size_t peak_x =
      size_t(std::clamp(std::round(fit_x), 0.0, double(width - 1)));
  const size_t peak_y =
      size_t(std::clamp(std::round(fit_y), 0.0, double(height - 1)));

  gaussian = schaapcommon::fitters::DeconvolveGaussian(gaussian, psf_parameters);
  log::Info() << "x=" << fit_x << ", y=" << fit_y << ", a=" << fit_a
              << ", maj=" << gaussian.major << ", min=" << gaussian.minor
              << ", pa=" << gaussian.position_angle << '\n';
  // The fitted component is not larger than the PSF (:283-289), or what is
  // left of it after the deconvolution is narrower than a pixel and cannot be
  // rendered on the grid: remove the central pixel as a point source.
  if (!std::isfinite(gaussian.major) || gaussian.major < kMinimumFwhm) {
    DeconvolvePointSource(peak_x, peak_y, data_image, model_image, psfs);
    return;
  }
  gaussian.minor = std::max(gaussian.minor, kMinimumFwhm);

  // the per-image values (:294-327): the Gaussian-weighted residual at the
  // peak over the Gaussian-weighted PSF at its centre, read directly instead
  // of through PsfCount() + Size() whole-image convolutions
  const size_t n_images = data_image.Size(), n_psfs = data_image.PsfCount();
  std::vector<float> component_values(n_images);
  {
    prof::Section prof_values("asp.weighted_values");
    std::vector<uint32_t> cx(std::max(n_images, n_psfs)), cy(cx.size());
    std::vector<double> psf_peaks(n_psfs), peaks(n_images);
    std::fill(cx.begin(), cx.end(), uint32_t(width / 2));
    std::fill(cy.begin(), cy.end(), uint32_t(height / 2));
    gpu::Check(rdl_gaussian_weighted_values(s, psfs.Base(), psfs.PlaneSize(), uint32_t(n_psfs),
                                            uint32_t(width), uint32_t(height), cx.data(),
                                            cy.data(), gaussian.major, gaussian.minor,
                                            gaussian.position_angle, psf_peaks.data()),
               "rdl_gaussian_weighted_values");
    std::fill(cx.begin(), cx.end(), uint32_t(peak_x));
    std::fill(cy.begin(), cy.end(), uint32_t(peak_y));
    gpu::Check(rdl_gaussian_weighted_values(s, data_image.Base(), data_image.PlaneSize(),
                                            uint32_t(n_images), uint32_t(width),
                                            uint32_t(height), cx.data(), cy.data(),
                                            gaussian.major, gaussian.minor,
                                            gaussian.position_angle, peaks.data()),
               "rdl_gaussian_weighted_values");
    for (size_t i = 0; i != n_images; ++i) {
      log::Debug() << "Component " << i << " peak: " << peaks[i] << '\n';
      component_values[i] = float(peaks[i] / psf_peaks[data_image.PsfIndex(i)]);
    }
  }
  PerformSpectralFit(component_values.data(), peak_x, peak_y);  // :329

  prof::Section prof_correct("asp.correct_and_model");
  for (size_t i = 0; i != n_images; ++i) {  // :332-370
    const double flux = double(component_values[i] * MinorLoopGain());
    gpu::Check(rdl_draw_gaussian(s, model_image.Data(i), uint32_t(width), uint32_t(height),
                                 fit_x, fit_y, gaussian.major, gaussian.minor,
                                 gaussian.position_angle, flux),
               "rdl_draw_gaussian");
    session_->Zero(scratch_->Ptr(), width * height * sizeof(float));
    gpu::Check(rdl_draw_gaussian(s, scratch_->F(), uint32_t(width), uint32_t(height), fit_x,
                                 fit_y, gaussian.major, gaussian.minor,
                                 gaussian.position_angle, flux),
               "rdl_draw_gaussian");
    CorrectResidual(data_image.Data(i), scratch_->F(), data_image.PsfIndex(i), psfs);
  }
}

void AspAlgorithm::CorrectResidual(float* d_residual, const float* d_component,
                                   size_t psf_index, const gpu::Planes& psfs) {
  gpu::Session& session = *session_;
  const size_t pw = padded_width_, ph = padded_height_;
  // one padded PSF spectrum per PSF and major iteration (:345-351 remake it
  // per component and image)
  auto it = psf_spectra_.find(psf_index);
  if (it == psf_spectra_.end())
    it = psf_spectra_
             .emplace(psf_index,
                      SubMinorLoop::MakeCorrectionPsfSpectrum(session, psfs.Plane(psf_index),
                                                              width_, height_, pw, ph))
             .first;
  const void* d_spectrum = it->second->Ptr();
  gpu::Fft& fft = session.GetFft(pw, ph, SubMinorLoop::CorrectionF64());
  if (fft.UsesLds()) {
    // Untrim, Convolve, Trim and the subtraction inside the transform passes
    gpu::Buffer& work =
        session.Scratch(gpu::Session::kCorrectionSpectrum, fft.ConvolveSubtractBytes());
    fft.ConvolveSubtract(d_component, width_, height_, (pw - width_) / 2, (ph - height_) / 2,
                         d_spectrum, work.Ptr(), d_residual, nullptr,
                         SubMinorLoop::CorrectionKernelF32() && fft.ConvColumnsD());
    return;
  }
  if (!padded_) padded_ = std::make_shared<gpu::Buffer>(session, pw * ph * sizeof(float));
  gpu::Check(rdl_untrim(session.Handle(), padded_->F(), uint32_t(pw), uint32_t(ph), d_component,
                        uint32_t(width_), uint32_t(height_)),
             "rdl_untrim");
  if (!fft.IsF64()) {
    fft.Convolve(padded_->F(), d_spectrum);
    gpu::Check(rdl_trim_subtract(session.Handle(), d_residual, uint32_t(width_),
                                 uint32_t(height_), padded_->F(), uint32_t(pw), uint32_t(ph)),
               "rdl_trim_subtract");
    return;
  }
  if (!padded_f64_)
    padded_f64_ = std::make_shared<gpu::Buffer>(session, pw * ph * sizeof(double));
  gpu::Check(rdl_convert(session.Handle(), padded_->Ptr(), padded_f64_->Ptr(), pw * ph, 1),
             "rdl_convert");
  fft.Convolve64(padded_f64_->D(), d_spectrum);
  gpu::Check(rdl_trim_subtract_f64(session.Handle(), d_residual, uint32_t(width_),
                                   uint32_t(height_), padded_f64_->D(), uint32_t(pw),
                                   uint32_t(ph)),
             "rdl_trim_subtract_f64");
}

}  // namespace radler::algorithms
