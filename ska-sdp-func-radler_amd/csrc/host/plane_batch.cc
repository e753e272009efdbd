// Line references are to the reference's cpp/radler.cc and
// cpp/algorithms/generic_clean.cc, whose single-image path every plane follows.
#include "plane_batch.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "clean_border.h"
#include "device.h"

namespace radler {

namespace {

[[noreturn]] void Refuse(const std::string& setting, const std::string& why) {
  throw std::runtime_error("PlaneBatch: settings." + setting + " " + why);
}

PlaneBatch::Planes HostPlanes(const std::vector<aocommon::Image>& images, size_t width,
                              size_t height, const char* name) {
  PlaneBatch::Planes planes;
  for (const aocommon::Image& image : images) {
    if (image.Width() != width || image.Height() != height)
      throw std::runtime_error(std::string("PlaneBatch: mismatch in ") + name + " image size");
    planes.planes.push_back(const_cast<float*>(image.Data()));
  }
  return planes;
}

PlaneBatch::Planes DevicePlanes(const std::vector<DeviceImage>& images, size_t width,
                                size_t height, const char* name) {
  PlaneBatch::Planes planes;
  planes.on_device = true;
  for (const DeviceImage& image : images) {
    if (image.width != width || image.height != height)
      throw std::runtime_error(std::string("PlaneBatch: mismatch in ") + name + " image size");
    if (!planes.planes.empty() && image.device != planes.device)
      throw std::runtime_error(std::string("PlaneBatch: the ") + name +
                               " images are on different HIP devices");
    planes.device = image.device;
    planes.planes.push_back(image.data);
  }
  return planes;
}

// The distance in elements between the planes of a device stack (0 for one
// plane); std::runtime_error when they are not evenly spaced.
size_t DeviceStride(const PlaneBatch::Planes& stack, size_t plane_size, const char* name) {
  if (stack.planes.size() < 2) return stack.planes.size() == 1 ? plane_size : 0;
  const std::ptrdiff_t stride = stack.planes[1] - stack.planes[0];
  for (size_t b = 1; b != stack.planes.size(); ++b)
    if (stack.planes[b] - stack.planes[b - 1] != stride || stride < std::ptrdiff_t(plane_size))
      throw std::runtime_error(std::string("PlaneBatch: the ") + name +
                               " planes in device memory are not one stack: a constant "
                               "distance of at least a plane between them is required");
  return size_t(stride);
}

}  // namespace

PlaneBatch::PlaneBatch(const Settings& settings, Planes psfs, Planes residuals, Planes models,
                       const std::vector<const uint8_t*>& masks)
    : settings_(settings),
      width_(settings.trimmed_image_width),
      height_(settings.trimmed_image_height),
      psfs_(std::move(psfs)),
      residuals_(std::move(residuals)),
      models_(std::move(models)) {
  Validate(masks.size());
  const size_t n = width_ * height_;
  n_masks_ = masks.size();
  masks_.resize(n_masks_ * n);
  for (size_t m = 0; m != n_masks_; ++m) {
    if (!masks[m]) throw std::runtime_error("PlaneBatch: a mask has no data");
    std::memcpy(masks_.data() + m * n, masks[m], n);
  }
  iterations_.assign(NPlanes(), 0);
  required_.assign(NPlanes(), true);
}

PlaneBatch::PlaneBatch(const Settings& settings, const std::vector<aocommon::Image>& psfs,
                       std::vector<aocommon::Image>& residuals,
                       std::vector<aocommon::Image>& models,
                       const std::vector<const uint8_t*>& masks)
    : PlaneBatch(settings,
                 HostPlanes(psfs, settings.trimmed_image_width, settings.trimmed_image_height,
                            "PSF"),
                 HostPlanes(residuals, settings.trimmed_image_width,
                            settings.trimmed_image_height, "residual"),
                 HostPlanes(models, settings.trimmed_image_width, settings.trimmed_image_height,
                            "model"),
                 masks) {}

PlaneBatch::PlaneBatch(const Settings& settings, const std::vector<DeviceImage>& psfs,
                       const std::vector<DeviceImage>& residuals,
                       const std::vector<DeviceImage>& models,
                       const std::vector<const uint8_t*>& masks)
    : PlaneBatch(settings,
                 DevicePlanes(psfs, settings.trimmed_image_width, settings.trimmed_image_height,
                              "PSF"),
                 DevicePlanes(residuals, settings.trimmed_image_width,
                              settings.trimmed_image_height, "residual"),
                 DevicePlanes(models, settings.trimmed_image_width,
                              settings.trimmed_image_height, "model"),
                 masks) {}

PlaneBatch::~PlaneBatch() = default;

int PlaneBatch::DeviceIndex() const {
  return settings_.gpu_device >= 0 ? settings_.gpu_device : gpu::Session::DefaultDevice();
}

void PlaneBatch::Validate(size_t n_masks) const {
  const Settings& s = settings_;
  // what a batch item is: one single-image Högbom clean
  if (s.algorithm_type != AlgorithmType::kGenericClean)
    Refuse("algorithm_type", "must be generic_clean: a batch item is a Högbom clean");
  if (s.generic.use_sub_minor_optimization)
    Refuse("generic.use_sub_minor_optimization", "must be false: a batch item is a Högbom clean");
  if (s.auto_mask_sigma) Refuse("auto_mask_sigma", "(auto-masking) is not available in a batch");
  if (s.absolute_auto_mask_threshold)
    Refuse("absolute_auto_mask_threshold", "(auto-masking) is not available in a batch");
  if (s.local_rms.method != LocalRmsMethod::kNone)
    Refuse("local_rms.method", "(local RMS) is not available in a batch");
  if (!s.local_rms.image.empty())
    Refuse("local_rms.image", "(local RMS) is not available in a batch");
  if (s.spectral_fitting.mode != schaapcommon::fitters::SpectralFittingMode::kNoFitting)
    Refuse("spectral_fitting.mode", "must be no_fitting: every plane is cleaned on its own");
  if (s.parallel.grid_width != 1) Refuse("parallel.grid_width", "must be 1");
  if (s.parallel.grid_height != 1) Refuse("parallel.grid_height", "must be 1");
  if (s.component_optimization_algorithm != OptimizationAlgorithm::kClean)
    Refuse("component_optimization_algorithm", "must be clean");
  if (!s.linked_polarizations.empty())
    Refuse("linked_polarizations", "must be empty: every plane is cleaned on its own");
  if (s.squared_joins) Refuse("squared_joins", "must be false: nothing is joined");
  if (!s.spectral_correction.empty())
    Refuse("spectral_correction", "must be empty: every plane is cleaned on its own");
  if (!s.fits_mask.empty()) Refuse("fits_mask", "is replaced by the masks argument");
  if (!s.casa_mask.empty()) Refuse("casa_mask", "is replaced by the masks argument");
  if (s.horizon_mask_distance)
    Refuse("horizon_mask_distance", "is replaced by the masks argument");
  if (s.save_source_list) Refuse("save_source_list", "is not available in a batch");
  if (width_ == 0 || height_ == 0)
    Refuse("trimmed_image_width", "and trimmed_image_height must be larger than zero");
  if (width_ > RDL_HOGBOM_BATCH_MAX_PIXELS || height_ > RDL_HOGBOM_BATCH_MAX_PIXELS ||
      width_ * height_ > RDL_HOGBOM_BATCH_MAX_PIXELS)
    Refuse("trimmed_image_width",
           "x trimmed_image_height is above 2^20 pixels: such a plane fills the device through "
           "Radler already");

  const size_t n_planes = residuals_.planes.size();
  if (n_planes == 0) throw std::runtime_error("PlaneBatch: nothing to clean");
  if (models_.planes.size() != n_planes)
    throw std::runtime_error("PlaneBatch: " + std::to_string(n_planes) + " residual planes and " +
                             std::to_string(models_.planes.size()) + " model planes");
  if (psfs_.planes.size() != 1 && psfs_.planes.size() != n_planes)
    throw std::runtime_error("PlaneBatch: one PSF or one per plane is required, " +
                             std::to_string(psfs_.planes.size()) + " given for " +
                             std::to_string(n_planes) + " planes");
  if (n_masks != 0 && n_masks != 1 && n_masks != n_planes)
    throw std::runtime_error("PlaneBatch: no mask, one mask or one per plane is required, " +
                             std::to_string(n_masks) + " given for " +
                             std::to_string(n_planes) + " planes");
  if (residuals_.on_device != models_.on_device)
    throw std::runtime_error(
        "PlaneBatch: residual and model planes must both be on the host or both on the device");
  for (const Planes* stack : {&psfs_, &residuals_, &models_}) {
    for (const float* plane : stack->planes)
      if (!plane) throw std::runtime_error("PlaneBatch: an image has no data");
    if (stack->on_device && stack->device != DeviceIndex())
      throw std::runtime_error("PlaneBatch: planes are on HIP device " +
                               std::to_string(stack->device) + ", the batch runs on device " +
                               std::to_string(DeviceIndex()));
  }
  const size_t n = width_ * height_;
  if (psfs_.on_device) DeviceStride(psfs_, n, "PSF");
  if (residuals_.on_device) {
    DeviceStride(residuals_, n, "residual");
    DeviceStride(models_, n, "model");
  }
}

void PlaneBatch::Perform(std::vector<bool>& another_iteration_required,
                         size_t major_iteration_number) {
  const size_t n_planes = NPlanes();
  const size_t n = width_ * height_;
  if (!session_) session_ = gpu::Session::ForDevice(DeviceIndex());
  gpu::Session& s = *session_;
  s.Bind();
  // Foreign device memory is read from here on, and its producer may have
  // used any stream: the whole device is waited for once, as Radler::Perform
  // does for its device images.
  const bool foreign = residuals_.on_device || psfs_.on_device;
  if (foreign) s.DeviceSync();

  std::vector<uint8_t> active(n_planes);
  for (size_t b = 0; b != n_planes; ++b) active[b] = !performed_ || required_[b];

  // ---- the stacks in device memory
  rdl_hogbom_batch_params p{};
  p.width = uint32_t(width_);
  p.height = uint32_t(height_);
  p.n_planes = uint32_t(n_planes);
  // ImageSet::LoadAndAverage for one entry of weight 1 turns -0 into +0
  p.flags = RDL_HOGBOM_BATCH_LOAD_RULE;
  if (psfs_.on_device) {
    p.d_psfs = psfs_.planes[0];
    p.psf_stride = psfs_.planes.size() == 1 ? 0 : DeviceStride(psfs_, n, "PSF");
  } else {
    if (!d_psfs_) {
      d_psfs_ = std::make_unique<gpu::Buffer>(s, psfs_.planes.size() * n * sizeof(float));
      for (size_t b = 0; b != psfs_.planes.size(); ++b)
        s.H2D(d_psfs_->F() + b * n, psfs_.planes[b], n * sizeof(float));
    }
    p.d_psfs = d_psfs_->F();
    p.psf_stride = psfs_.planes.size() == 1 ? 0 : n;
  }
  if (residuals_.on_device) {
    p.d_residuals = residuals_.planes[0];
    p.residual_stride = DeviceStride(residuals_, n, "residual");
    p.d_models = models_.planes[0];
    p.model_stride = DeviceStride(models_, n, "model");
  } else {
    if (!d_residuals_) {
      d_residuals_ = std::make_unique<gpu::Buffer>(s, n_planes * n * sizeof(float));
      d_models_ = std::make_unique<gpu::Buffer>(s, n_planes * n * sizeof(float));
    }
    for (size_t b = 0; b != n_planes; ++b) {
      if (!active[b]) continue;
      s.H2D(d_residuals_->F() + b * n, residuals_.planes[b], n * sizeof(float));
      s.H2D(d_models_->F() + b * n, models_.planes[b], n * sizeof(float));
    }
    p.d_residuals = d_residuals_->F();
    p.residual_stride = n;
    p.d_models = d_models_->F();
    p.model_stride = n;
  }
  if (n_masks_ != 0) {
    if (!d_masks_) {
      d_masks_ = std::make_unique<gpu::Buffer>(s, masks_.size());
      s.H2D(d_masks_->Ptr(), masks_.data(), masks_.size());
    }
    p.d_mask = static_cast<const uint8_t*>(d_masks_->Ptr());
    p.mask_stride = n_masks_ == 1 ? 0 : n;
  }

  // ---- the algorithm's settings, with InitializeDeconvolutionAlgorithm's
  // conversions to float (:368-375)
  p.gain = float(settings_.minor_loop_gain);
  p.major_loop_gain = float(settings_.major_loop_gain);
  p.divergence_limit = float(settings_.divergence_limit);
  // generic_clean.cc:111: stopping on a negative component allows them
  p.allow_negative =
      settings_.allow_negative_components || settings_.stop_on_negative_components;
  p.stop_on_negative = settings_.stop_on_negative_components;
  const algorithms::Borders border =
      algorithms::CleanBorders(width_, height_, float(settings_.border_ratio));
  p.h_border = border.horizontal;
  p.v_border = border.vertical;

  // ---- the threshold of each plane (:228-244 without auto-masking and with
  // threshold_bias = 0: squared joins are refused)
  std::vector<float> threshold(n_planes, float(settings_.absolute_threshold));
  if (settings_.auto_threshold_sigma) {
    for (size_t b = 0; b != n_planes; ++b) {
      if (!active[b]) continue;
      // integrated.MedianAndStdDevFromMAD() (:162-166); the integrated image
      // of one entry of weight 1 is the plane itself
      const float* plane = p.d_residuals + b * p.residual_stride;
      float med = 0.0f, mad = 0.0f;
      gpu::Check(rdl_median(s.Handle(), plane, n, 0, 0.0f, &med), "rdl_median");
      gpu::Check(rdl_median(s.Handle(), plane, n, 1, med, &mad), "rdl_median");
      const double stddev = double(mad) * 1.48260221850560;
      threshold[b] = float(
          std::max(stddev * (*settings_.auto_threshold_sigma), settings_.absolute_threshold));
    }
  }

  std::vector<uint64_t> iteration_start(iterations_.begin(), iterations_.end());
  const std::vector<uint64_t> max_iterations(n_planes, settings_.minor_iteration_count);
  std::vector<rdl_hogbom_batch_out> out(n_planes);
  gpu::Check(rdl_hogbom_batch_run(s.Handle(), &p, threshold.data(), iteration_start.data(),
                                  max_iterations.data(), active.data(), out.data(), nullptr, 0),
             "rdl_hogbom_batch_run");

  if (!residuals_.on_device) {
    for (size_t b = 0; b != n_planes; ++b) {
      if (!active[b]) continue;
      s.D2H(residuals_.planes[b], d_residuals_->F() + b * n, n * sizeof(float));
      s.D2H(models_.planes[b], d_models_->F() + b * n, n * sizeof(float));
    }
  }

  // ---- generic_clean.cc:122-136 and :230-248, then the caps of
  // radler.cc:287-308, per plane
  another_iteration_required.assign(n_planes, false);
  const float major_loop_gain = float(settings_.major_loop_gain);
  for (size_t b = 0; b != n_planes; ++b) {
    if (!active[b]) continue;
    const rdl_hogbom_batch_out& o = out[b];
    bool another = false;
    const bool ran = o.start.found && iteration_start[b] < settings_.minor_iteration_count;
    if (ran && !o.result.diverging && o.result.found) {
      const float initial_max_value = std::fabs(o.start.value);
      const float major_iter_threshold =
          std::max(0.0f, initial_max_value * (1.0f - major_loop_gain));
      const float peak = o.result.peak;
      const bool final_threshold_reached = std::fabs(peak) <= threshold[b] || peak == 0.0f;
      const bool negative_reached = peak < 0.0f && settings_.stop_on_negative_components;
      const bool mgain_reached = std::fabs(peak) <= major_iter_threshold;
      const bool did_work = o.result.iteration != iteration_start[b];
      another = mgain_reached && did_work && !negative_reached && !final_threshold_reached;
    }
    iterations_[b] = size_t(o.result.iteration);
    if (another && settings_.major_iteration_count != 0 &&
        major_iteration_number >= settings_.major_iteration_count)
      another = false;
    if (another && settings_.minor_iteration_count != 0 &&
        iterations_[b] >= settings_.minor_iteration_count)
      another = false;
    another_iteration_required[b] = another;
  }
  required_ = another_iteration_required;
  performed_ = true;
  // every store to device images is complete: any stream may consume them
  if (foreign) s.Sync();
}

}  // namespace radler
