// MultiScaleAlgorithm on the device. Line references are to the reference's
// cpp/algorithms/multiscale_algorithm.cc unless stated.
#include "multiscale_algorithm.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <optional>
#include <set>
#include <stdexcept>

#include "communicator.h"
#include "component_optimization.h"
#include "fft_sizes.h"
#include "host_profile.h"
#include "logger.h"
#include "scale_search.h"
#include "subminor.h"

namespace radler::algorithms {

using multiscale::MultiScaleTransforms;

namespace {
// The switches of the environment. All but RDL_SUBMINOR_DEFER are read at the
// start of every major iteration (MultiScaleAlgorithm::Switches), so a test
// can compare both sides in one process.
// RDL_SCALE_LANES=1: the scales' inverse transforms on one stream (default 2)
int ScaleLanes() {
  const char* e = std::getenv("RDL_SCALE_LANES");
  return e && e[0] == '1' ? 1 : 2;
}

// RDL_FUSED_SCALES=0: the scales' convolutions through the forward spectrum
// and one two-pass column inverse each instead of the fused multi-scale
// launch (for comparisons)
bool FusedScalesOn() {
  const char* e = std::getenv("RDL_FUSED_SCALES");
  return !(e && e[0] == '0');
}

// RDL_SUBMINOR_DEFER=0: read each sub-minor loop's result before queuing the
// correction (comparison; read once per process)
bool DeferLoopResult() {
  static const bool on = [] {
    const char* e = std::getenv("RDL_SUBMINOR_DEFER");
    return !(e && e[0] == '0');
  }();
  return on;
}

// RDL_CORR_PEAK=0: the scale-0 peak search reads the corrected residual
// again instead of running inside the correction's inverse row pass
bool CorrPeakOn() {
  const char* e = std::getenv("RDL_CORR_PEAK");
  return !(e && e[0] == '0');
}

// RDL_PSF_CACHE=0: the scale-convolved PSFs and the padded PSF spectra are
// made again in every major iteration; RDL_PSF_CACHE_MB: what the kept ones
// may hold (default 16384; what does not fit is made again as without)
bool PsfCacheOn() {
  const char* e = std::getenv("RDL_PSF_CACHE");
  return !(e && e[0] == '0');
}

size_t PsfCacheBudget() {
  const char* e = std::getenv("RDL_PSF_CACHE_MB");
  char* end = nullptr;
  const unsigned long long mb = e ? std::strtoull(e, &end, 10) : 16384ull;
  return size_t(e && end == e ? 16384ull : mb) << 20;
}

// RDL_MODEL_GATE=0: the scale > 0 model update chooses between stamping and
// the FFT by the loop's selected pixels instead of its components
bool ModelGateOn() {
  const char* e = std::getenv("RDL_MODEL_GATE");
  return !(e && e[0] == '0');
}
}  // namespace

void InitializeScales(std::vector<MultiScaleAlgorithm::ScaleInfo>& scales,
                      double beam_size_in_pixels, size_t min_width_height,
                      MultiscaleShape shape, size_t max_scales,
                      const std::vector<double>& scale_list) {  // :90-131
  if (scale_list.empty()) {
    if (scales.empty()) {
      size_t scale_index = 0;
      double scale = beam_size_in_pixels * 2.0;
      do {
        MultiScaleAlgorithm::ScaleInfo& e = scales.emplace_back();
        e.scale = scale_index == 0 ? 0.0f : float(scale);
        e.kernel_peak =
            MultiScaleTransforms::KernelPeakValue(scale, min_width_height, shape);
        scale *= 2.0;
        ++scale_index;
      } while (scale < min_width_height * 0.5 &&
               (max_scales == 0 || scale_index < max_scales));
    } else {
      while (!scales.empty() && scales.back().scale >= min_width_height * 0.5) {
        log::Info() << "Scale size " << scales.back().scale
                    << " does not fit in cleaning region: removing scale.\n";
        scales.pop_back();
      }
    }
  } else if (scales.empty()) {
    std::multiset<double> sorted(scale_list.begin(), scale_list.end());
    for (double s : sorted) {
      MultiScaleAlgorithm::ScaleInfo& e = scales.emplace_back();
      e.scale = float(s);
      e.kernel_peak =
          MultiScaleTransforms::KernelPeakValue(e.scale, min_width_height, shape);
    }
  }
}

std::optional<size_t> SelectMaximumScale(
    const std::vector<MultiScaleAlgorithm::ScaleInfo>& scales) {  // :133-151
  std::map<float, size_t> peak_to_scale;
  for (size_t i = 0; i != scales.size(); ++i)
    if (scales[i].is_active)
      peak_to_scale.insert(std::make_pair(
          std::fabs(scales[i].max_unnormalized_image_value *
                    scales[i].bias_factor),
          i));
  if (peak_to_scale.empty()) return std::nullopt;
  return peak_to_scale.rbegin()->second;
}

MultiScaleAlgorithm::MultiScaleAlgorithm(const Settings::Multiscale& settings,
                                         double beam_size, double pixel_scale_x,
                                         double pixel_scale_y,
                                         bool track_components)
    : settings_(settings),
      beam_size_in_pixels_(beam_size / std::max(pixel_scale_x, pixel_scale_y)),
      track_components_(track_components) {
  if (!(beam_size_in_pixels_ > 0.0)) beam_size_in_pixels_ = 1;  // :162
}

MultiScaleAlgorithm::MultiScaleAlgorithm(const MultiScaleAlgorithm& o)
    : DeconvolutionAlgorithm(o),
      settings_(o.settings_),
      beam_size_in_pixels_(o.beam_size_in_pixels_),
      track_components_(o.track_components_),
      component_list_(o.component_list_ ? std::make_unique<ComponentList>(*o.component_list_)
                                        : nullptr),
      scale_infos_(o.scale_infos_),
      track_masks_(o.track_masks_),
      use_masks_(o.use_masks_),
      host_masks_(o.host_masks_) {}

void MultiScaleAlgorithm::UploadScaleMasks(gpu::Session& s, size_t n_pixels) {
  if (!masks_dirty_ && masks_session_ == &s && dev_masks_.size() == host_masks_.size())
    return;
  dev_masks_.clear();
  for (const std::vector<uint8_t>& m : host_masks_) {
    gpu::Buffer& b = dev_masks_.emplace_back(s, n_pixels);
    if (m.size() == n_pixels)
      s.H2D(b.Ptr(), m.data(), n_pixels);
    else
      b.Zero();
  }
  masks_session_ = &s;
  masks_dirty_ = false;
}

void MultiScaleAlgorithm::DownloadScaleMasks() {
  if (!masks_session_) return;
  for (size_t i = 0; i != host_masks_.size() && i != dev_masks_.size(); ++i)
    masks_session_->D2H(host_masks_[i].data(), dev_masks_[i].Ptr(), host_masks_[i].size());
}

void MultiScaleAlgorithm::RunFullComponentFitter(ImageSet& residual_set,
                                                 ImageSet& model_set,
                                                 const gpu::Planes& psfs) {
  // :916-929 over the images, :837-914 per image
  if (ComponentOptimizationAlgorithm() != OptimizationAlgorithm::kGradientDescent)
    throw std::runtime_error(
        "Unsupported optimization algorithm for multiscale clean algorithm");
  if (!component_list_)
    throw std::runtime_error(
        "Multiscale component optimisation fits the component list: it needs "
        "save_source_list");
  gpu::Session& s = residual_set.Session();
  const size_t width = residual_set.Width(), height = residual_set.Height();
  EnsureTransforms(transforms_, s, width, height, settings_.shape);
  std::vector<float> scales;
  std::vector<std::vector<std::pair<size_t, size_t>>> lists(scale_infos_.size());
  for (size_t sc = 0; sc != scale_infos_.size(); ++sc) {
    scales.push_back(scale_infos_[sc].scale);
    if (sc < component_list_->NScales())
      for (size_t i = 0; i != component_list_->ComponentCount(sc); ++i)
        lists[sc].push_back(component_list_->GetComponentPosition(sc, i));
  }
  const size_t pw = utils::GetConvolutionSize(scales.back(), width,
                                              settings_.convolution_padding);
  const size_t ph = utils::GetConvolutionSize(scales.back(), height,
                                              settings_.convolution_padding);
  std::vector<float> model(width * height);
  for (size_t i = 0; i != residual_set.Size(); ++i) {
    // :885-897 ("Updating component list") runs before :898-905 ("Updating
    // model"): the list values take the model image's values from before
    // this fit's deltas are added
    s.D2H(model.data(), model_set.Data(i), model.size() * sizeof(float));
    for (size_t sc = 0; sc != lists.size(); ++sc)
      for (size_t c = 0; c != lists[sc].size(); ++c)
        component_list_->Value(sc, c, i) +=
            model[lists[sc][c].second * width + lists[sc][c].first];
    math::RunFullComponentFitter(s, residual_set.Data(i), model_set.Data(i),
                                 psfs.Plane(residual_set.PsfIndex(i)), width, height, scales,
                                 lists, *transforms_, pw, ph);
  }
  // ApplySpectralConstraintsToComponents (deconvolution_algorithm.cc:48-64)
  std::vector<float> values(component_list_->NFrequencies());
  for (size_t sc = 0; sc != component_list_->NScales(); ++sc)
    for (size_t c = 0; c != component_list_->ComponentCount(sc); ++c) {
      size_t x, y;
      component_list_->GetComponent(sc, c, x, y, values.data());
      PerformSpectralFit(values.data(), x, y);
      for (size_t f = 0; f != values.size(); ++f) component_list_->Value(sc, c, f) = values[f];
    }
}

const float* MultiScaleAlgorithm::PeakSearchInput(const float* d_image, size_t w,
                                                 size_t h) {
  if (!RmsFactorImage()) return d_image;
  if (!rms_scratch_ || rms_scratch_->Bytes() < w * h * sizeof(float))
    rms_scratch_ = std::make_shared<gpu::Buffer>(*session_, w * h * sizeof(float));
  return RmsWeighted(*session_, d_image, rms_scratch_->F(), w, h);
}

float MultiScaleAlgorithm::Normalized(float value, size_t x, size_t y, size_t w) const {
  if (!RmsFactorImage()) return value;
  return value / (*RmsFactorImage())[x + y * w];
}

void MultiScaleAlgorithm::FindPeakDirect(const float* d_image,
                                         size_t scale_index) {  // :700-748
  prof::Section prof_section("ms.find_peak_direct");
  const size_t w = transforms_->Width(), h = transforms_->Height();
  d_image = PeakSearchInput(d_image, w, h);
  const Borders border = PeakBorders(w, h);
  rdl_peak p;
  gpu::Check(rdl_find_peak(session_->Handle(), d_image, uint32_t(w), uint32_t(h), 0,
                           uint32_t(h), border.horizontal, border.vertical,
                           AllowNegativeComponents(), MaskFor(scale_index), 1, &p),
             "rdl_find_peak");
  StorePeak(scale_infos_[scale_index], p,
            [&](float v, size_t x, size_t y) { return Normalized(v, x, y, w); });
}

float* MultiScaleAlgorithm::KeptScaleImage(size_t scale_index, size_t w, size_t h) {
  gpu::Planes& kept = scale_images_[scale_index];
  if (!kept.buffer || kept.width != w || kept.height != h)
    kept = gpu::Planes::Make(*session_, w, h, 1);
  return kept.Base();
}

void MultiScaleAlgorithm::FindActiveScaleConvolvedMaxima(
    const ImageSet& image_set, float* d_integrated, bool report_rms) {
  prof::Section prof_section("ms.find_maxima");
  // :578-634 with ThreadedDeconvolutionTools::FindMultiScalePeak /
  // FindSingleScalePeak (threaded_deconvolution_tools.cc:30-107): one forward
  // FFT of the integrated image feeds every active scale.
  rdl_session* s = session_->Handle();
  const size_t w = image_set.Width(), h = image_set.Height();
  auto normalized = [&](float v, size_t x, size_t y) { return Normalized(v, x, y, w); };

  // The source. One image whose integration is the identity: the searches and
  // the forward transform read the residual itself (no integrated copy), and
  // every scale's convolved image is kept for IndividualImages.
  const bool identity = image_set.Size() == 1 && image_set.Integration(false).copy_fast_path;
  scale_image_valid_.assign(scale_infos_.size(), false);
  if (identity && scale_images_.size() != scale_infos_.size())
    scale_images_.assign(scale_infos_.size(), gpu::Planes());
  const float* d_source = d_integrated;
  if (identity)
    d_source = image_set.Data(0);
  else
    image_set.GetLinearIntegrated(d_integrated);
  // A reported RMS and the RMS-weighted search read the convolved image (the
  // search a weighted copy of it), so those searches are not fused into the
  // inverse row pass and scale 0 is searched at once.
  const bool fused_search = !report_rms && !RmsFactorImage();
  // the scale-0 search the residual correction already queued in slot 0
  const bool scale0_queued = scale0_search_queued_;
  scale0_search_queued_ = false;

  // Scale 0 is searched as it is (FindPeakDirect, :700-748): queued with the
  // convolved scales' searches (one read-back for all) when those are queued
  // too. Every allocation is made here, before any lane is forked.
  int direct = -1;
  std::vector<ConvolvedScale> convolved;
  for (size_t si = 0; si != scale_infos_.size(); ++si) {
    ScaleInfo& e = scale_infos_[si];
    if (!e.is_active) continue;
    if (e.scale != 0.0f) {
      float* d_image = scratch_->F();
      if (identity) {
        d_image = KeptScaleImage(si, w, h);
        scale_image_valid_[si] = true;
      }
      convolved.push_back({si, e.scale, d_image, MaskFor(si), PeakBorders(w, h, e.scale),
                           report_rms ? &e.rms : nullptr});
    } else if (fused_search) {
      direct = int(si);
    } else {
      FindPeakDirect(d_source, si);
      if (report_rms) gpu::Check(rdl_rms(s, d_source, w * h, &e.rms), "rdl_rms");
    }
  }
  if (convolved.empty()) {  // scale 0 alone
    if (direct >= 0 && scale0_queued)
      CollectPeaks(s, {size_t(direct)}, scale_infos_, normalized);
    else if (direct >= 0)
      FindPeakDirect(d_source, size_t(direct));
    return;
  }
  if (scale_infos_.size() + 1 > RDL_PEAK_SLOTS)
    throw std::runtime_error("MultiScaleAlgorithm: too many scales");
  std::vector<size_t> pending;  // scale of each queued peak search (slot = index)
  if (direct >= 0) {
    const Borders border = PeakBorders(w, h);
    if (!scale0_queued)
      gpu::Check(rdl_find_peak_enqueue(s, d_source, uint32_t(w), uint32_t(h), 0, uint32_t(h),
                                       border.horizontal, border.vertical,
                                       AllowNegativeComponents(), MaskFor(size_t(direct)), 1, 0),
                 "rdl_find_peak_enqueue");
    pending.push_back(size_t(direct));
  }

  // two lanes only with one image per scale (identity: kept images)
  const bool two_lanes = identity && fused_search && spectrum_work2_ && convolved.size() > 1;
  ScaleSearch search{*session_,
                     *transforms_,
                     spectrum_->Ptr(),
                     {spectrum_work_->Ptr(), spectrum_work2_ ? spectrum_work2_->Ptr() : nullptr},
                     scale_u_,
                     AllowNegativeComponents()};
  if (fused_search && switches_.fused_scales && transforms_->Fused())
    search.Fused(d_source, convolved, two_lanes, pending);
  else
    search.ThroughSpectrum(d_source, convolved, fused_search, two_lanes, pending,
                           [&](const float* d_image) { return PeakSearchInput(d_image, w, h); });
  CollectPeaks(s, pending, scale_infos_, normalized);
}

void MultiScaleAlgorithm::ActivateScales(size_t last) {  // :636-656
  for (size_t i = 0; i != scale_infos_.size(); ++i) {
    const bool activate =
        i == last ||
        std::fabs(scale_infos_[i].max_unnormalized_image_value) *
                scale_infos_[i].bias_factor >
            std::fabs(scale_infos_[last].max_unnormalized_image_value) *
                (1.0 - MinorLoopGain()) * scale_infos_[last].bias_factor;
    scale_infos_[i].is_active = activate;
  }
}

void MultiScaleAlgorithm::SetUpScalesAndMasks(ImageSet& data_image) {
  const size_t width = data_image.Width(), height = data_image.Height();
  const size_t npx = width * height;
  InitializeScales(scale_infos_, beam_size_in_pixels_, std::min(width, height),
                   settings_.shape, settings_.max_scales, settings_.scale_list);
  if (track_components_) {  // :228-236
    if (!component_list_)
      component_list_ = std::make_unique<ComponentList>(width, height, scale_infos_.size(),
                                                        data_image.Size());
    else if (component_list_->Width() != width || component_list_->Height() != height)
      throw std::runtime_error("Error in component list dimensions!");
  }
  if (track_masks_) {  // :214-226
    for (const std::vector<uint8_t>& m : host_masks_)
      if (m.size() != npx)
        throw std::runtime_error("Invalid automask size in multiscale algorithm");
    while (host_masks_.size() < scale_infos_.size()) {
      host_masks_.emplace_back(npx, 0);
      masks_dirty_ = true;
    }
  }
  if (track_masks_ || use_masks_) UploadScaleMasks(data_image.Session(), npx);
}

gpu::Buffer MultiScaleAlgorithm::SetUpBuffers(ImageSet& data_image) {
  gpu::Session& session = data_image.Session();
  const size_t width = data_image.Width(), height = data_image.Height();
  EnsureTransforms(transforms_, session, width, height, settings_.shape, &scale_infos_);
  d_mask_ = DeviceCleanMask(session, width, height);
  scratch_ = std::make_shared<gpu::Buffer>(session, width * height * sizeof(float));
  gpu::Buffer integrated(session, width * height * sizeof(float));
  const size_t spectrum_bytes = transforms_->SpectrumBytes();
  spectrum_ = std::make_shared<gpu::Buffer>(session, spectrum_bytes);
  spectrum_work_ = std::make_shared<gpu::Buffer>(session, spectrum_bytes);
  spectrum_work2_.reset();
  scale_u_.clear();
  // the second lane only on a main session: a subimage pool's workers
  // already keep up to 16 streams busy, and a lane pair per worker adds
  // a spectrum buffer and fork/join events to every small subimage
  if (switches_.scale_lanes > 1 && !session.IsWorker() && data_image.Size() == 1 &&
      data_image.Integration(false).copy_fast_path)
    spectrum_work2_ = std::make_shared<gpu::Buffer>(session, spectrum_bytes);
  return integrated;
}

void MultiScaleAlgorithm::SetUpScalePsfs() {
  const double first_auto_scale_size = beam_size_in_pixels_ * 2.0;
  const size_t n_scales = scale_infos_.size();
  for (size_t si = 0; si != n_scales; ++si) {
    ScaleInfo& e = scale_infos_[si];
    e.psf_peak = psf_products_.PsfPeak(si);
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

void MultiScaleAlgorithm::SharePlanes(const Iteration& it, ImageSet& set) {
  if (!it.sharded) return;
  prof::Section prof_share("ms.shard_broadcast");
  const size_t plane_bytes = set.Width() * set.Height() * sizeof(float);
  for (size_t i = 0; i != set.Size(); ++i)
    shard_->Broadcast(*session_, set.Data(i), plane_bytes, it.Owner(i));
}

bool MultiScaleAlgorithm::StartThresholds(Iteration& it, const ScaleInfo& first) {
  bool is_final_threshold = false;
  it.initial_peak_value = std::fabs(first.max_unnormalized_image_value * first.bias_factor);
  float m_gain_threshold = it.initial_peak_value * (1.0 - MajorLoopGain());
  m_gain_threshold = std::max(m_gain_threshold, MajorIterationThreshold());
  it.first_threshold = m_gain_threshold;
  if (Threshold() > it.first_threshold) {
    it.first_threshold = Threshold();
    is_final_threshold = true;
  }
  log::Info() << "Starting multi-scale cleaning. Start peak=" << it.initial_peak_value
              << ", major iteration threshold=" << it.first_threshold
              << (is_final_threshold ? " (final)\n" : "\n");
  return is_final_threshold;
}

float MultiScaleAlgorithm::SubIterationThreshold(Iteration& it, const ScaleInfo& info) {
  const float sub_iteration_gain_threshold =
      std::fabs(info.max_unnormalized_image_value * info.bias_factor) *
      (1.0 - settings_.sub_minor_loop_gain);
  float first_sub_iteration_threshold = sub_iteration_gain_threshold;
  if (it.first_threshold > first_sub_iteration_threshold) {
    first_sub_iteration_threshold = it.first_threshold;
    if (!it.has_hit_threshold_in_sub_loop) {
      log::Info() << "Subminor loop is near minor loop threshold. "
                     "Initiating countdown.\n";
      it.has_hit_threshold_in_sub_loop = true;
    }
    it.threshold_countdown--;
  }
  return first_sub_iteration_threshold;
}

void MultiScaleAlgorithm::IndividualImages(ImageSet& individual, const ImageSet& data_image,
                                           size_t scale_index) {  // :336-354
  const float scale = scale_infos_[scale_index].scale;
  if (scale != 0.0f && scale_index < scale_image_valid_.size() &&
      scale_image_valid_[scale_index]) {
    // the residual has not changed since FindActiveScaleConvolvedMaxima
    // convolved it with this scale: take that image
    gpu::Planes previous = individual.Planes();
    individual.SetPlanes(scale_images_[scale_index]);
    scale_images_[scale_index] = previous;
    scale_image_valid_[scale_index] = false;
  } else if (!(settings_.fast_sub_minor_loop && scale == 0.0f)) {
    // (at scale 0 the fast sub-minor loop only reads the images, so it reads
    // the residual itself)
    individual.CopyFrom(data_image);
    if (scale != 0.0f)
      for (size_t i = 0; i != data_image.Size(); ++i)
        transforms_->Transform(individual.Data(i), scale);
  }
}

void MultiScaleAlgorithm::ConfigureSubMinorLoop(SubMinorLoop& sub, Iteration& it,
                                                size_t scale_index, float threshold) {
  gpu::Session& session = *session_;
  const ScaleInfo& info = scale_infos_[scale_index];
  const size_t width = it.data.Width(), height = it.data.Height();
  sub.SetIterationInfo(IterationNumber(), MaxIterations());
  sub.SetThreshold(threshold / info.bias_factor);
  sub.SetGain(info.gain);
  sub.SetDivergenceLimit(DivergenceLimit());
  sub.SetAllowNegativeComponents(AllowNegativeComponents());
  sub.SetStopOnNegativeComponent(StopOnNegativeComponents());
  const Borders border = PeakBorders(width, height, info.scale);
  sub.SetCleanBorders(border.horizontal, border.vertical);
  sub.SetMask(MaskFor(scale_index));
  sub.SetSpectralMap(DeviceSpectralMap(session, it.data.Size()));
  sub.SetLogPolyFit(DeviceFit(session, width, height));
  sub.SetRmsFactor(DeviceRmsFactor(session, width, height));  // :401-402
}

void MultiScaleAlgorithm::Account(Iteration& it, SubMinorLoop& sub, ScaleInfo& info,
                                  size_t sub_start, const SubMinorLoop::RunResult& result) {
  it.diverging = result.diverging;
  if (DivergenceLimit() != 0.0f)
    it.diverging = it.diverging ||
                   std::fabs(result.peak) > it.initial_peak_value * DivergenceLimit();
  SetIterationNumber(sub.CurrentIteration());
  info.n_components_cleaned += IterationNumber() - sub_start;
  info.total_flux_cleaned += sub.FluxCleaned();
}

std::optional<gpu::PeakRequest> MultiScaleAlgorithm::Scale0PeakRequest(
    const ImageSet& data_image) const {
  std::optional<gpu::PeakRequest> request;
  if (!switches_.corr_peak || data_image.Size() != 1 ||
      !data_image.Integration(false).copy_fast_path || RmsFactorImage())
    return request;
  for (size_t si = 0; si != scale_infos_.size(); ++si)
    if (scale_infos_[si].is_active && scale_infos_[si].scale == 0.0f) {
      const Borders border = PeakBorders(data_image.Width(), data_image.Height());
      gpu::PeakRequest& q = request.emplace();
      q.h_border = border.horizontal;
      q.v_border = border.vertical;
      q.allow_negative = AllowNegativeComponents();
      q.d_mask = MaskFor(si);
      q.slot = 0;
      break;
    }
  return request;
}

void MultiScaleAlgorithm::AddScaleModel(Iteration& it, SubMinorLoop& sub, float scale,
                                        size_t sub_start, size_t i) {
  // The scale > 0 model update: stamping the shape kernel costs
  // n^2 multiply-adds per component (the stamping kernel skips the
  // selected pixels whose model value stayed zero), against two
  // full-image FFTs (:451-460 convolves with the same kernel). The
  // loop's component count is known once its result is read, so a
  // deferred loop's update is queued after that; the loop never reads
  // the model image.
  size_t n_kernel = 0;
  const float* d_kernel = transforms_->ShapeKernel(scale, n_kernel);
  size_t n_stamps = sub.NSelected();
  if (switches_.model_gate) n_stamps = std::min(n_stamps, IterationNumber() - sub_start);
  if (double(n_stamps) * double(n_kernel) * double(n_kernel) <= 1e9) {
    sub.AddShapeModel(i, d_kernel, n_kernel, it.model.Data(i));
  } else {
    sub.GetFullIndividualModel(i, scratch_->F());
    transforms_->Transform(scratch_->F(), scale);
    gpu::Check(rdl_add(session_->Handle(), it.model.Data(i), scratch_->F(),
                       it.model.Width() * it.model.Height()),
               "rdl_add");
  }
}

void MultiScaleAlgorithm::CorrectAndModel(Iteration& it, SubMinorLoop& sub, size_t scale_index,
                                          size_t sub_start, size_t conv_w, size_t conv_h,
                                          bool model_after_result) {  // :436-462
  prof::Section prof_correct("ms.correct_and_model");
  const float scale = scale_infos_[scale_index].scale;
  if (track_masks_ && scale_index < dev_masks_.size())  // :444-445
    sub.UpdateAutoMask(static_cast<uint8_t*>(dev_masks_[scale_index].Ptr()));
  // The scales of the next searches (:521) follow from the previous
  // searches' results alone, so they are known before the correction is
  // queued. With scale 0 among them, and one image that is its own
  // integrated image searched unweighted, the correction's inverse row
  // pass makes that search over the residual values as it writes them
  // (peak slot 0) instead of a pass that reads the residual again.
  ActivateScales(scale_index);
  const std::optional<gpu::PeakRequest> scale0_peak = Scale0PeakRequest(it.data);
  for (size_t i = 0; i != it.data.Size(); ++i) {
    if (it.Owner(i) != it.my_rank) continue;  // another rank's image
    const gpu::Buffer& padded =
        psf_products_.PaddedSpectrum(it.data.PsfIndex(i), scale_index, conv_w, conv_h);
    if (sub.CorrectResidualDirtyWithSpectrum(i, it.data.Data(i), padded.Ptr(),
                                             scale0_peak ? &*scale0_peak : nullptr))
      scale0_search_queued_ = true;
    if (scale == 0.0f)
      sub.AddIndividualModel(i, it.model.Data(i));
    else if (!model_after_result)
      AddScaleModel(it, sub, scale, sub_start, i);
  }
  if (track_components_)  // :447-448
    sub.UpdateComponentList(*component_list_, scale_index);
}

bool MultiScaleAlgorithm::FastSubMinorStep(Iteration& it, size_t scale_index, float threshold,
                                           ImageSet& individual, const gpu::Planes& twice,
                                           bool& searched) {  // :377-462
  ScaleInfo& info = scale_infos_[scale_index];
  const size_t width = it.data.Width(), height = it.data.Height();
  const size_t sub_start = IterationNumber();
  const size_t conv_w =
      utils::GetConvolutionSize(info.scale, width, settings_.convolution_padding);
  const size_t conv_h =
      utils::GetConvolutionSize(info.scale, height, settings_.convolution_padding);
  SubMinorLoop sub(*session_, width, height, conv_w, conv_h);
  ConfigureSubMinorLoop(sub, it, scale_index, threshold);
  std::vector<uint32_t> xy;
  if (RecordTrace()) sub.SetTrace(&xy);
  // Without a trace or a component list, the loop's result (its
  // component count, last peak, divergence) is read only after the work
  // that does not depend on it is queued: the correction, the model
  // update and the next peak searches (:436-462, :521-524) run behind the
  // loop on the stream instead of after a host round trip.
  const bool defer = !RecordTrace() && !track_components_ && DeferLoopResult();
  // at scale 0 the loop only reads the images, so it reads the residual itself
  ImageSet& images = info.scale == 0.0f ? it.data : individual;
  SubMinorLoop::RunResult r;
  {
    prof::Section prof_run("ms.subminor_run");
    if (defer)
      r = {false, sub.Launch(images, twice), 0.0f};
    else
      r = sub.Run(images, twice);
  }
  for (size_t c = 0; c + 1 < xy.size(); c += 2) {
    trace_.push_back(xy[c]);
    trace_.push_back(xy[c + 1]);
    trace_.push_back(uint32_t(scale_index));
  }
  if (!r.has_peak) {
    log::Warn() << "Could not continue multi-scale clean, because the "
                   "sub-minor loop failed to find components.\n";
    return false;
  }
  if (!defer) Account(it, sub, info, sub_start, r);
  // a deferred loop's scale > 0 model update waits for its component count
  const bool model_after_result = defer && switches_.model_gate && info.scale != 0.0f;
  CorrectAndModel(it, sub, scale_index, sub_start, conv_w, conv_h, model_after_result);
  SharePlanes(it, it.data);  // the corrected residuals, from their owners
  if (defer) {
    FindActiveScaleConvolvedMaxima(it.data, it.d_integrated, false);
    searched = true;
    Account(it, sub, info, sub_start, sub.Collect());
    if (model_after_result) {
      prof::Section prof_model("ms.correct_and_model");
      for (size_t i = 0; i != it.data.Size(); ++i)
        if (it.Owner(i) == it.my_rank) AddScaleModel(it, sub, info.scale, sub_start, i);
    }
  }
  return true;
}

void MultiScaleAlgorithm::SlowSubMinorStep(Iteration& it, size_t scale_index, float threshold,
                                           ImageSet& individual,
                                           const gpu::Planes& twice) {  // :463-519
  gpu::Session& session = *session_;
  rdl_session* s = session.Handle();
  ScaleInfo& info = scale_infos_[scale_index];
  ImageSet& data_image = it.data;
  const size_t width = data_image.Width(), height = data_image.Height();
  size_t n_kernel = 0;
  std::vector<float> shape_kernel;
  if (info.scale != 0.0f)
    shape_kernel = MultiScaleTransforms::MakeShapeFunction(
        info.scale, n_kernel, std::min(width, height), settings_.shape);
  else
    shape_kernel = {1.0f}, n_kernel = 1;
  std::vector<float> cv(data_image.Size());
  while (IterationNumber() < MaxIterations() &&
         std::fabs(info.max_unnormalized_image_value * info.bias_factor) > threshold &&
         (!StopOnNegativeComponents() || info.max_unnormalized_image_value >= 0.0) &&
         !it.diverging) {
    const size_t x = info.max_image_value_x, y = info.max_image_value_y;
    for (size_t i = 0; i != data_image.Size(); ++i)
      cv[i] = session.ReadFloat(individual.Data(i) + x + y * width);
    PerformSpectralFit(cv.data(), x, y);  // :477
    trace_.push_back(uint32_t(x));
    trace_.push_back(uint32_t(y));
    trace_.push_back(uint32_t(scale_index));
    for (size_t i = 0; i != data_image.Size(); ++i) {
      cv[i] = cv[i] * info.gain;
      const size_t pi = data_image.PsfIndex(i);
      gpu::Check(rdl_subtract_psf(s, data_image.Data(i),
                                  psf_products_.Convolved(pi).Plane(scale_index),
                                  uint32_t(width), uint32_t(height), uint32_t(x), uint32_t(y),
                                  cv[i]),
                 "rdl_subtract_psf");
      gpu::Check(rdl_subtract_psf(s, individual.Data(i), twice.Plane(pi), uint32_t(width),
                                  uint32_t(height), uint32_t(x), uint32_t(y), cv[i]),
                 "rdl_subtract_psf");
      // AddComponentToModel (:676-698): scale 0 adds the value itself
      // (fma(1, v, m) == m + v), larger scales stamp the shape kernel.
      gpu::Check(rdl_add_shape_component(s, it.model.Data(i), uint32_t(width), uint32_t(height),
                                         shape_kernel.data(), uint32_t(n_kernel), uint32_t(x),
                                         uint32_t(y), cv[i]),
                 "rdl_add_shape_component");
      info.n_components_cleaned++;
      info.total_flux_cleaned += cv[i];
      if (track_masks_ && scale_index < dev_masks_.size()) {  // :695-696
        const uint8_t one = 1;
        session.H2D(static_cast<uint8_t*>(dev_masks_[scale_index].Ptr()) + x + width * y, &one,
                    1);
      }
    }
    if (track_components_)  // :502-504
      component_list_->Add(x, y, scale_index, cv.data());
    individual.GetLinearIntegrated(it.d_integrated);
    FindPeakDirect(it.d_integrated, scale_index);
    const float abs_peak = std::fabs(info.max_unnormalized_image_value * info.bias_factor);
    if (DivergenceLimit() != 0.0f)
      it.diverging = abs_peak > it.initial_peak_value * DivergenceLimit();
    SetIterationNumber(IterationNumber() + 1);
  }
}

void MultiScaleAlgorithm::LogScalePeaks() const {
  char buf[256];
  std::string line = "[ms] it=" + std::to_string(IterationNumber());
  for (const ScaleInfo& e : scale_infos_) {
    std::snprintf(buf, sizeof(buf), " | s=%g a=%d v=%.9g x=%zu y=%zu", e.scale,
                  int(e.is_active), e.max_unnormalized_image_value * e.bias_factor,
                  e.max_image_value_x, e.max_image_value_y);
    line += buf;
  }
  std::fprintf(stderr, "%s\n", line.c_str());
}

DeconvolutionResult MultiScaleAlgorithm::ExecuteMajorIteration(
    ImageSet& data_image, ImageSet& model_image, const gpu::Planes& psfs) {
  prof::Section prof_section("ms.execute");
  gpu::Session& session = data_image.Session();
  session_ = &session;
  switches_ = {ScaleLanes(), FusedScalesOn(), CorrPeakOn(), PsfCacheOn(), ModelGateOn(),
               PsfCacheBudget()};  // Switches' order
  const size_t width = data_image.Width();
  const size_t height = data_image.Height();
  trace_.clear();
  scale0_search_queued_ = false;
  if (StopOnNegativeComponents()) SetAllowNegativeComponents(true);
  SetUpScalesAndMasks(data_image);
  MaskSync mask_sync{this};
  if (ComponentOptimizationAlgorithm() != OptimizationAlgorithm::kClean) {  // :242-246
    RejectForcedTermsForOptimization();
    RunFullComponentFitter(data_image, model_image, psfs);
    return DeconvolutionResult{};
  }

  const int n_ranks = shard_ ? shard_->Size() : 1;
  Iteration it{data_image, model_image, nullptr, n_ranks, shard_ ? shard_->Rank() : 0,
               n_ranks > 1 && data_image.Size() > 1};
  it.threshold_countdown = std::max(size_t{8}, scale_infos_.size() * 3 / 2);
  gpu::Buffer integrated = SetUpBuffers(data_image);
  it.d_integrated = integrated.F();

  // ConvolvePsfs (:29-88): a main session keeps the products for the next
  // major iteration; otherwise they go when this call returns.
  MultiScalePsfProducts::IterationGuard products_guard{psf_products_};
  {
    prof::Section prof_integrate("ms.integrate_psf");
    data_image.GetIntegratedPsf(integrated.F(), psfs);
  }
  std::vector<float> scales;
  for (const ScaleInfo& e : scale_infos_) scales.push_back(e.scale);
  psf_products_.Begin({session, *transforms_, width, height, scales, settings_.shape,
                       settings_.convolution_padding, data_image.PsfCount(), integrated.F(),
                       psfs},
                      switches_.psf_cache && !session.IsWorker(), switches_.psf_cache_budget);
  SetUpScalePsfs();

  FindActiveScaleConvolvedMaxima(data_image, integrated.F(), true);
  DeconvolutionResult result;
  std::optional<size_t> optional_scale = SelectMaximumScale(scale_infos_);
  if (!optional_scale) {
    log::Warn() << "No peak found during multi-scale cleaning! Aborting "
                   "deconvolution.\n";
    result.another_iteration_required = false;
    return result;
  }
  size_t scale_with_peak = *optional_scale;
  const bool is_final_threshold = StartThresholds(it, scale_infos_[scale_with_peak]);

  ImageSet individual(data_image, width, height);
  while (IterationNumber() < MaxIterations() &&
         std::fabs(scale_infos_[scale_with_peak].max_unnormalized_image_value *
                   scale_infos_[scale_with_peak].bias_factor) > it.first_threshold &&
         (!StopOnNegativeComponents() ||
          scale_infos_[scale_with_peak].max_unnormalized_image_value >= 0.0) &&
         it.threshold_countdown > 0 && !it.diverging) {  // :323-543
    bool searched = false;  // the next peak searches already ran (deferred result)
    const gpu::Planes& twice = psf_products_.Twice(scale_with_peak);
    IndividualImages(individual, data_image, scale_with_peak);
    const float threshold = SubIterationThreshold(it, scale_infos_[scale_with_peak]);
    if (!settings_.fast_sub_minor_loop)
      SlowSubMinorStep(it, scale_with_peak, threshold, individual, twice);
    else if (!FastSubMinorStep(it, scale_with_peak, threshold, individual, twice, searched))
      break;

    if (!searched) {
      ActivateScales(scale_with_peak);
      FindActiveScaleConvolvedMaxima(data_image, integrated.F(), false);
    }
    if (log::Verbosity() >= 3) LogScalePeaks();
    optional_scale = SelectMaximumScale(scale_infos_);
    if (!optional_scale) {
      log::Warn() << "No peak found in main loop of multi-scale cleaning! "
                     "Aborting deconvolution.\n";
      result.another_iteration_required = false;
      SharePlanes(it, model_image);
      return result;
    }
    scale_with_peak = *optional_scale;
    log::Info() << "Iteration " << IterationNumber() << ", scale "
                << std::round(scale_infos_[scale_with_peak].scale) << " px : "
                << scale_infos_[scale_with_peak].max_unnormalized_image_value *
                       scale_infos_[scale_with_peak].bias_factor
                << " at " << scale_infos_[scale_with_peak].max_image_value_x
                << ',' << scale_infos_[scale_with_peak].max_image_value_y << '\n';
  }

  const bool max_iter_reached = IterationNumber() >= MaxIterations();
  const bool negative_reached =
      StopOnNegativeComponents() &&
      scale_infos_[scale_with_peak].max_unnormalized_image_value < 0.0;
  if (it.diverging)
    log::Warn() << "WARNING: Multiscale clean diverged.\n";
  result.is_diverging = it.diverging;
  result.another_iteration_required =
      !max_iter_reached && !is_final_threshold && !negative_reached && !it.diverging;
  result.final_peak_value =
      scale_infos_[scale_with_peak].max_unnormalized_image_value *
      scale_infos_[scale_with_peak].bias_factor;
  SharePlanes(it, model_image);  // the owners' model updates
  session.Sync();
  return result;
}

}  // namespace radler::algorithms
