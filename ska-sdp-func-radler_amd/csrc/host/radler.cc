// Line references are to the reference's cpp/radler.cc.
#include "radler.h"

#include "host_profile.h"

#include <cmath>
#include <sstream>
#include <stdexcept>

#include "asp_algorithm.h"
#include "device.h"
#include "fits_image.h"
#include "generic_clean.h"
#include "image_accessors.h"
#include "image_set.h"
#include "logger.h"
#include "iuwt_deconvolution.h"
#include "multiscale_algorithm.h"
#include "parallel_deconvolution.h"
#include "python_deconvolution_factory.h"
#include "rms_image.h"

namespace radler {

namespace {
[[noreturn]] void Unsupported(const char* what) {
  throw std::runtime_error(std::string(what) +
                           " is not available in the MI355X build of Radler");
}
}  // namespace

Radler::Radler(const Settings& settings, std::unique_ptr<WorkTable> table,
               double beam_size)
    : Radler(settings, beam_size) {
  InitializeDeconvolutionAlgorithm(std::move(table));
}

Radler::Radler(const Settings& settings, const aocommon::Image& psf_image,
               aocommon::Image& residual_image, aocommon::Image& model_image,
               double beam_size, aocommon::PolarizationEnum polarization)
    : Radler(settings, beam_size) {
  // :52-91
  if (psf_image.Width() != settings.trimmed_image_width ||
      psf_image.Height() != settings.trimmed_image_height)
    throw std::runtime_error("Mismatch in PSF image size");
  if (residual_image.Width() != settings.trimmed_image_width ||
      residual_image.Height() != settings.trimmed_image_height)
    throw std::runtime_error("Mismatch in residual image size");
  if (model_image.Width() != settings.trimmed_image_width ||
      model_image.Height() != settings.trimmed_image_height)
    throw std::runtime_error("Mismatch in model image size");
  auto table = std::make_unique<WorkTable>(std::vector<PsfOffset>{}, 1, 1);
  auto e = std::make_unique<WorkTableEntry>();
  e->polarization = polarization;
  e->image_weight = 1.0;
  e->psf_accessors.emplace_back(
      std::make_unique<utils::LoadOnlyImageAccessor>(psf_image));
  e->residual_accessor =
      std::make_unique<utils::LoadAndStoreImageAccessor>(residual_image);
  e->model_accessor =
      std::make_unique<utils::LoadAndStoreImageAccessor>(model_image);
  table->AddEntry(std::move(e));
  InitializeDeconvolutionAlgorithm(std::move(table));
}

Radler::Radler(const Settings& settings, const DeviceImage& psf_image,
               const DeviceImage& residual_image, const DeviceImage& model_image,
               double beam_size, aocommon::PolarizationEnum polarization)
    : Radler(settings, beam_size) {
  if (psf_image.width != settings.trimmed_image_width ||
      psf_image.height != settings.trimmed_image_height)
    throw std::runtime_error("Mismatch in PSF image size");
  if (residual_image.width != settings.trimmed_image_width ||
      residual_image.height != settings.trimmed_image_height)
    throw std::runtime_error("Mismatch in residual image size");
  if (model_image.width != settings.trimmed_image_width ||
      model_image.height != settings.trimmed_image_height)
    throw std::runtime_error("Mismatch in model image size");
  if (!psf_image.data || !residual_image.data || !model_image.data)
    throw std::runtime_error("Radler: a device image has no data");
  auto table = std::make_unique<WorkTable>(std::vector<PsfOffset>{}, 1, 1);
  auto e = std::make_unique<WorkTableEntry>();
  e->polarization = polarization;
  e->image_weight = 1.0;
  const auto accessor = [](const DeviceImage& image, bool writable) {
    return std::make_unique<utils::DeviceImageAccessor>(image.data, image.width, image.height,
                                                        image.device, writable);
  };
  e->psf_accessors.emplace_back(accessor(psf_image, false));
  e->residual_accessor = accessor(residual_image, true);
  e->model_accessor = accessor(model_image, true);
  table->AddEntry(std::move(e));
  InitializeDeconvolutionAlgorithm(std::move(table));
}

Radler::Radler(const Settings& settings, double beam_size)
    : settings_(settings),
      image_width_(settings.trimmed_image_width),
      image_height_(settings.trimmed_image_height),
      pixel_scale_x_(settings.pixel_scale.x),
      pixel_scale_y_(settings.pixel_scale.y),
      beam_size_(beam_size) {
  // :93-117
  if (settings.spectral_fitting.mode ==
          schaapcommon::fitters::SpectralFittingMode::kForcedTerms &&
      settings.spectral_fitting.forced_filename.empty())
    throw std::runtime_error(
        "Forced fitting filename is required when forced fitting is enabled.");
  if (settings.parallel.grid_width == 0)
    throw std::runtime_error("parallel.grid_width must be larger than zero");
  if (settings.parallel.grid_height == 0)
    throw std::runtime_error("parallel.grid_height must be larger than zero");
  if (settings.parallel.max_threads == 0)
    throw std::runtime_error("parallel.max_threads must be larger than zero");
  parallel_deconvolution_ =
      std::make_unique<algorithms::ParallelDeconvolution>(settings_);
}

Radler::~Radler() { FreeDeconvolutionAlgorithms(); }

ComponentList Radler::GetComponentList() const {
  // ParallelDeconvolution::GetComponentList (parallel_deconvolution.cc:185-210)
  if (settings_.algorithm_type == AlgorithmType::kMultiscale)
    return parallel_deconvolution_->GetMultiscaleComponentList();
  ImageSet model_set(*table_, settings_.squared_joins,
                     settings_.linked_polarizations, image_width_,
                     image_height_, DeviceSession());
  // the model planes' producer may have used any stream
  if (has_device_images_) DeviceSession().DeviceSync();
  model_set.LoadAndAverage(false);
  ComponentList list(image_width_, image_height_, model_set);
  list.MergeDuplicates();
  return list;
}

const algorithms::DeconvolutionAlgorithm& Radler::MaxScaleCountAlgorithm()
    const {
  return parallel_deconvolution_->MaxScaleCountAlgorithm();
}

void Radler::Perform(bool& another_iteration_required,
                     size_t major_iteration_number) {  // :130-316
  if (!table_) throw std::runtime_error("Radler: not initialized");
  prof::Section prof_total("perform.total");
  table_->ValidatePsfs();
  log::Info() << " == Deconvolving (" << major_iteration_number << ") ==\n";
  gpu::Session& s = DeviceSession();
  ImageSet residual_set(*table_, settings_.squared_joins,
                        settings_.linked_polarizations, image_width_,
                        image_height_, s);
  ImageSet model_set(*table_, settings_.squared_joins,
                     settings_.linked_polarizations, image_width_,
                     image_height_, s);
  // Foreign device memory is read from here on, and its producer may have
  // used any stream: the whole device is waited for once.
  if (has_device_images_) s.DeviceSync();
  {
    prof::Section p("perform.load");
    residual_set.LoadAndAverage(true);
    model_set.LoadAndAverage(false);
  }

  const bool auto_mask_is_enabled =
      settings_.auto_mask_sigma || settings_.absolute_auto_mask_threshold;
  // an RMS image file takes precedence over a constructed one (:189-196)
  const bool rms_from_file = !settings_.local_rms.image.empty();
  const bool local_rms =
      !rms_from_file && settings_.local_rms.method != LocalRmsMethod::kNone;
  const size_t n_px = image_width_ * image_height_;
  gpu::Buffer integrated;
  double median = 0.0, stddev = 0.0;
  if (settings_.auto_threshold_sigma || auto_mask_is_enabled || local_rms) {
    // integrated.MedianAndStdDevFromMAD() (:162-166) on the device
    integrated = gpu::Buffer(s, n_px * sizeof(float));
    residual_set.GetLinearIntegrated(integrated.F());
    float med = 0.0f, mad = 0.0f;
    gpu::Check(rdl_median(s.Handle(), integrated.F(), n_px, 0, 0.0f, &med), "rdl_median");
    gpu::Check(rdl_median(s.Handle(), integrated.F(), n_px, 1, med, &mad), "rdl_median");
    median = med;
    stddev = double(mad) * 1.48260221850560;
    log::Info() << "Estimated standard deviation of background noise: "
                << stddev << '\n';
  }
  if (auto_mask_is_enabled && auto_mask_is_finished_) {
    // :172-185: once the auto-mask is complete a more aggressive gain is
    // used, and the RMS background no longer
    parallel_deconvolution_->SetMinorLoopGain(
        std::min(1.0, settings_.minor_loop_gain * 2.0));
    parallel_deconvolution_->SetRmsFactorImage(nullptr, image_width_);
    // component optimisation only once the mask is complete (:180-185)
    if (settings_.component_optimization_algorithm != OptimizationAlgorithm::kClean)
      parallel_deconvolution_->SetComponentOptimization(
          settings_.component_optimization_algorithm);
  } else {
    parallel_deconvolution_->SetMinorLoopGain(settings_.minor_loop_gain);
    if (rms_from_file) {  // :189-195
      if (rms_file_image_.empty()) {
        FitsImageReader reader(settings_.local_rms.image, "Local RMS image file");
        if (reader.Width() != image_width_ || reader.Height() != image_height_)
          throw std::runtime_error(
              "The local RMS image '" + settings_.local_rms.image +
              "' does not have the dimensions of the deconvolved image");
        rms_file_image_.resize(n_px);
        reader.ReadIndex(rms_file_image_.data(), 0);
      }
      gpu::Buffer rms(s, n_px * sizeof(float));
      s.H2D(rms.Ptr(), rms_file_image_.data(), n_px * sizeof(float));
      stddev = math::rms_image::MakeRmsFactorImage(s, rms.F(), n_px,
                                                   settings_.local_rms.strength);
      auto factor = std::make_shared<std::vector<float>>(n_px);
      s.D2H(factor->data(), rms.F(), n_px * sizeof(float));
      parallel_deconvolution_->SetRmsFactorImage(std::move(factor), image_width_);
    } else if (local_rms) {  // :196-216
      gpu::Buffer rms(s, n_px * sizeof(float));
      if (settings_.local_rms.method == LocalRmsMethod::kRmsWindow)
        math::rms_image::Make(s, rms.F(), integrated.F(), image_width_, image_height_,
                              settings_.local_rms.window, beam_size_, beam_size_, 0.0,
                              pixel_scale_x_, pixel_scale_y_);
      else
        math::rms_image::MakeWithNegativityLimit(
            s, rms.F(), integrated.F(), image_width_, image_height_,
            settings_.local_rms.window, beam_size_, beam_size_, 0.0, pixel_scale_x_,
            pixel_scale_y_);
      stddev = math::rms_image::MakeRmsFactorImage(s, rms.F(), n_px,
                                                   settings_.local_rms.strength);
      log::Info() << "Lowest RMS in image: " << stddev << '\n';
      auto factor = std::make_shared<std::vector<float>>(n_px);
      s.D2H(factor->data(), rms.F(), n_px * sizeof(float));
      parallel_deconvolution_->SetRmsFactorImage(std::move(factor), image_width_);
    }
  }
  // :228-243
  const double threshold_bias = settings_.squared_joins ? median : 0.0;
  if (auto_mask_is_enabled && !auto_mask_is_finished_) {
    const double combined_auto_mask_threshold =
        std::max(stddev * settings_.auto_mask_sigma.value_or(0.0) + threshold_bias,
                 settings_.absolute_auto_mask_threshold.value_or(0.0));
    parallel_deconvolution_->SetThreshold(
        std::max(combined_auto_mask_threshold, settings_.absolute_threshold));
  } else if (settings_.auto_threshold_sigma) {
    parallel_deconvolution_->SetThreshold(
        std::max(stddev * (*settings_.auto_threshold_sigma) + threshold_bias,
                 settings_.absolute_threshold));
  }

  // :249-275: multiscale tracks per-scale masks until the auto-mask
  // threshold is reached, then cleans inside them; the other algorithms get
  // the scale-independent mask of the model's non-zero pixels
  if (settings_.algorithm_type == AlgorithmType::kMultiscale) {
    if (auto_mask_is_enabled)
      parallel_deconvolution_->SetAutoMaskMode(!auto_mask_is_finished_,
                                               auto_mask_is_finished_);
  } else if (auto_mask_is_enabled && auto_mask_is_finished_) {
    if (auto_mask_.empty()) {
      auto_mask_.assign(image_width_ * image_height_, 0);
      std::vector<float> plane(image_width_ * image_height_);
      for (size_t i = 0; i != model_set.Size(); ++i) {
        s.D2H(plane.data(), model_set.Data(i), plane.size() * sizeof(float));
        for (size_t p = 0; p != plane.size(); ++p)
          if (std::isfinite(plane[p]) && plane[p] != 0.0f) auto_mask_[p] = 1;
      }
    }
    parallel_deconvolution_->SetCleanMask(reinterpret_cast<const bool*>(auto_mask_.data()));
  }

  std::vector<gpu::Planes> psf_images;
  {
    prof::Section p("perform.load_psfs");
    psf_images = residual_set.LoadAndAveragePsfs();
  }
  algorithms::ParallelDeconvolutionResult result;
  {
    prof::Section p("perform.execute");
    result = parallel_deconvolution_->ExecuteMajorIteration(
        residual_set, model_set, psf_images, table_->PsfOffsets(),
        settings_.major_loop_gain);
  }
  another_iteration_required = result.another_iteration_required;

  if (!another_iteration_required && auto_mask_is_enabled && !auto_mask_is_finished_) {
    log::Info() << "Auto-masking threshold reached; continuing next major "
                   "iteration with deeper threshold and mask.\n";
    auto_mask_is_finished_ = true;
    another_iteration_required = true;
    auto_mask_finishing_iteration_ = major_iteration_number;
  }
  if (another_iteration_required && settings_.major_iteration_count != 0 &&
      major_iteration_number >= settings_.major_iteration_count) {
    another_iteration_required = false;
    log::Info() << "Maximum number of major iterations was reached: not "
                   "continuing deconvolution.\n";
  }
  if (another_iteration_required && auto_mask_is_finished_ &&
      major_iteration_number - auto_mask_finishing_iteration_ >=
          settings_.major_auto_mask_iteration_count) {
    another_iteration_required = false;
    log::Info() << "Performed "
                << major_iteration_number - auto_mask_finishing_iteration_
                << " major iterations after reaching the auto-mask threshold: "
                   "not continuing deconvolution.\n";
  }
  if (another_iteration_required && settings_.minor_iteration_count != 0 &&
      parallel_deconvolution_->FirstAlgorithm().IterationNumber() >=
          settings_.minor_iteration_count) {
    another_iteration_required = false;
    log::Info() << "Maximum number of minor deconvolution iterations was "
                   "reached: not continuing deconvolution.\n";
  }
  prof::Section prof_store("perform.store");
  residual_set.AssignAndStoreResidual();
  const algorithms::DeconvolutionAlgorithm& first =
      parallel_deconvolution_->FirstAlgorithm();
  model_set.InterpolateAndStoreModel(first.HasSpectralFitter() ? &first.Fitter() : nullptr,
                                     first.SpectrallyForcedImages().get());
  // every store to device images is complete: any stream may consume them
  if (has_device_images_) s.Sync();
}

std::unique_ptr<schaapcommon::fitters::SpectralFitter>
Radler::CreateSpectralFitter() const {  // :318-331
  std::vector<double> channel_frequencies;
  std::vector<float> channel_weights;
  if (settings_.spectral_fitting.mode !=
      schaapcommon::fitters::SpectralFittingMode::kNoFitting)
    ImageSet::CalculateDeconvolutionFrequencies(*table_, channel_frequencies,
                                                channel_weights);
  return std::make_unique<schaapcommon::fitters::SpectralFitter>(
      settings_.spectral_fitting.mode, settings_.spectral_fitting.terms,
      std::move(channel_frequencies), std::move(channel_weights));
}

void Radler::InitializeDeconvolutionAlgorithm(
    std::unique_ptr<WorkTable> table) {  // :333-395
  FreeDeconvolutionAlgorithms();
  table_ = std::move(table);
  if (table_->OriginalGroups().empty()) throw std::runtime_error("Nothing to clean");
  has_device_images_ = ImageSet::HasDeviceAccessors(*table_);
  if (has_device_images_) ValidateDeviceImages();
  if (!std::isfinite(beam_size_)) {
    log::Warn() << "No proper beam size available in deconvolution!\n";
    beam_size_ = 0.0;
  }
  if (!settings_.casa_mask.empty()) Unsupported("A CASA mask (casacore table input)");
  std::unique_ptr<algorithms::DeconvolutionAlgorithm> algorithm;
  switch (settings_.algorithm_type) {
    case AlgorithmType::kGenericClean:
      algorithm = std::make_unique<algorithms::GenericClean>(
          settings_.generic.use_sub_minor_optimization);
      break;
    case AlgorithmType::kMultiscale:
      algorithm = std::make_unique<algorithms::MultiScaleAlgorithm>(
          settings_.multiscale, beam_size_, pixel_scale_x_, pixel_scale_y_,
          settings_.save_source_list);
      break;
    case AlgorithmType::kIuwt:
      algorithm = std::make_unique<algorithms::IuwtDeconvolution>();
      break;
    case AlgorithmType::kAdaptiveScalePixel:  // :355-358
      algorithm = std::make_unique<algorithms::AspAlgorithm>(
          settings_.multiscale, beam_size_, pixel_scale_x_, pixel_scale_y_);
      break;
    case AlgorithmType::kMoreSane:
      Unsupported("MoreSane");
    case AlgorithmType::kPython:  // :371-374; hosted by the Python module
      algorithm = algorithms::MakePythonDeconvolution(settings_.python.filename);
      break;
  }
  algorithm->SetMaxIterations(settings_.minor_iteration_count);
  algorithm->SetThreshold(settings_.absolute_threshold);
  algorithm->SetMinorLoopGain(settings_.minor_loop_gain);
  algorithm->SetMajorLoopGain(settings_.major_loop_gain);
  algorithm->SetCleanBorderRatio(settings_.border_ratio);
  algorithm->SetDivergenceLimit(settings_.divergence_limit);
  algorithm->SetAllowNegativeComponents(settings_.allow_negative_components);
  algorithm->SetStopOnNegativeComponents(settings_.stop_on_negative_components);
  algorithm->SetSpectralFitter(CreateSpectralFitter(),
                               table_->OriginalGroups().front().size());
  parallel_deconvolution_->SetAlgorithm(std::move(algorithm));
  if (settings_.spectral_fitting.mode ==
      schaapcommon::fitters::SpectralFittingMode::kForcedTerms)
    ReadForcedSpectrumImages();
  ReadMask(*table_);
}

void Radler::ReadForcedSpectrumImages() {  // :410-432
  if (settings_.component_optimization_algorithm != OptimizationAlgorithm::kClean)
    throw std::runtime_error(
        "Component optimization cannot be combined with forced-term spectral fitting");
  log::Debug() << "Reading " << settings_.spectral_fitting.forced_filename << ".\n";
  FitsImageReader reader(settings_.spectral_fitting.forced_filename, "Forced spectrum file");
  if (reader.Width() != image_width_ || reader.Height() != image_height_)
    throw std::runtime_error(
        "The image dimensions of the forced spectrum fits file do not match "
        "the deconvolved image dimensions");
  if (reader.NImages() + 1 != settings_.spectral_fitting.terms)
    throw std::runtime_error(
        "The number of images in the forced spectrum fits file does not match "
        "the deconvolved image dimensions");
  std::vector<std::vector<float>> terms(reader.NImages());
  for (size_t t = 0; t != terms.size(); ++t) {
    terms[t].resize(image_width_ * image_height_);
    reader.ReadIndex(terms[t].data(), t);
  }
  parallel_deconvolution_->SetSpectrallyForcedImages(std::move(terms), image_width_);
}

void Radler::ReadMask(const WorkTable& group_table) {  // :434-527
  const size_t n_px = image_width_ * image_height_;
  bool has_mask = false;
  if (!settings_.fits_mask.empty()) {
    FitsImageReader mask_reader(settings_.fits_mask, "Fits mask file");
    if (mask_reader.Width() != image_width_ || mask_reader.Height() != image_height_)
      throw std::runtime_error(
          "Specified Fits file mask did not have same dimensions as output "
          "image!");
    std::vector<float> mask_data(n_px);
    if (mask_reader.NFrequencies() == 1) {
      log::Debug() << "Reading mask '" << settings_.fits_mask << "'...\n";
      mask_reader.ReadIndex(mask_data.data(), 0);
    } else if (mask_reader.NFrequencies() == settings_.channels_out) {
      const size_t index = group_table.Front().mask_channel_index;
      log::Debug() << "Reading mask '" << settings_.fits_mask << "' (" << (index + 1)
                   << ")...\n";
      mask_reader.ReadIndex(mask_data.data(), index);
    } else {
      std::stringstream msg;
      msg << "The number of frequencies in the specified fits mask ("
          << mask_reader.NFrequencies()
          << ") does not match the number of requested output channels ("
          << settings_.channels_out << ")";
      throw std::runtime_error(msg.str());
    }
    clean_mask_.assign(n_px, 0);
    for (size_t i = 0; i != n_px; ++i) clean_mask_[i] = mask_data[i] != 0.0f ? 1 : 0;
    has_mask = true;
  }

  if (settings_.horizon_mask_distance) {  // :484-524
    if (!has_mask) {
      clean_mask_.assign(n_px, 1);
      has_mask = true;
    }
    double fov_sq = M_PI_2 - *settings_.horizon_mask_distance;
    if (fov_sq < 0.0) fov_sq = 0.0;
    if (fov_sq <= M_PI_2) {
      fov_sq = std::sin(fov_sq);
    } else {  // a negative horizon distance was given
      fov_sq = 1.0 - *settings_.horizon_mask_distance;
    }
    fov_sq = fov_sq * fov_sq;
    uint8_t* ptr = clean_mask_.data();
    for (size_t y = 0; y != image_height_; ++y) {
      for (size_t x = 0; x != image_width_; ++x) {
        double l, m;
        aocommon::ImageCoordinates::XYToLM(x, y, pixel_scale_x_, pixel_scale_y_,
                                           image_width_, image_height_, l, m);
        if (l * l + m * m >= fov_sq) *ptr = 0;
        ++ptr;
      }
    }
    log::Info() << "Saving horizon mask...\n";
    std::vector<float> image(n_px);
    for (size_t i = 0; i != n_px; ++i) image[i] = clean_mask_[i] ? 1.0f : 0.0f;
    std::string filename = settings_.horizon_mask_filename;
    if (filename.empty()) filename = settings_.prefix_name + "-horizon-mask.fits";
    WriteFitsImage(filename, image.data(), image_width_, image_height_,
                   settings_.pixel_scale.x, settings_.pixel_scale.y);
  }
  if (has_mask)
    parallel_deconvolution_->SetCleanMask(reinterpret_cast<const bool*>(clean_mask_.data()));
}

int Radler::DeviceIndex() const {
  return settings_.gpu_device >= 0 ? settings_.gpu_device : gpu::Session::DefaultDevice();
}

void Radler::ValidateDeviceImages() const {
  const int device = DeviceIndex();
  struct Range {
    const char* begin;
    const char* end;
    std::string name;
  };
  std::vector<Range> residuals, models;
  const auto check = [&](const aocommon::ImageAccessor* accessor, const std::string& name,
                         bool is_psf, std::vector<Range>* ranges) {
    const auto* image = dynamic_cast<const utils::DeviceImageAccessor*>(accessor);
    if (!image) return;
    std::ostringstream msg;
    if (image->Device() != device) {
      msg << "Radler: the " << name << " is on HIP device " << image->Device()
          << ", the deconvolution runs on device " << device;
      throw std::runtime_error(msg.str());
    }
    if (is_psf) return;  // sizes: WorkTable::ValidatePsfs
    if (image->Width() != image_width_ || image->Height() != image_height_) {
      msg << "Radler: the " << name << " is " << image->Width() << " x " << image->Height()
          << " pixels, the settings give " << image_width_ << " x " << image_height_;
      throw std::runtime_error(msg.str());
    }
    if (!image->Writable()) {
      msg << "Radler: the " << name << " (device " << image->Device() << ", address "
          << static_cast<const void*>(image->Data())
          << ") is read-only, Perform() writes residual and model images";
      throw std::runtime_error(msg.str());
    }
    const char* begin = reinterpret_cast<const char*>(image->Data());
    ranges->push_back(Range{begin, begin + image->Bytes(), name});
  };
  for (const WorkTableEntry& e : *table_) {
    const std::string of_entry = " image of entry " + std::to_string(e.index);
    check(e.residual_accessor.get(), "residual" + of_entry, false, &residuals);
    check(e.model_accessor.get(), "model" + of_entry, false, &models);
    for (size_t p = 0; p != e.psf_accessors.size(); ++p)
      check(e.psf_accessors[p].get(), "PSF " + std::to_string(p) + of_entry, true, nullptr);
  }
  for (const Range& r : residuals)
    for (const Range& m : models)
      if (r.begin < m.end && m.begin < r.end) {
        std::ostringstream msg;
        msg << "Radler: the " << r.name << " [" << static_cast<const void*>(r.begin) << ", "
            << static_cast<const void*>(r.end) << ") overlaps the " << m.name << " ["
            << static_cast<const void*>(m.begin) << ", " << static_cast<const void*>(m.end)
            << ") in device memory";
        throw std::runtime_error(msg.str());
      }
}

void Radler::FreeDeconvolutionAlgorithms() {
  parallel_deconvolution_->FreeDeconvolutionAlgorithms();
  table_.reset();
}

void Radler::SetCommunicator(std::shared_ptr<Communicator> comm) {
  parallel_deconvolution_->SetCommunicator(std::move(comm));
}

gpu::Session& Radler::DeviceSession() const {
  // The device is opened on first use, so constructing a Radler (argument
  // validation) needs no GPU; Perform() fails loudly without one.
  if (!session_) {
    session_ = gpu::Session::ForDevice(DeviceIndex());
  }
  return *session_;
}

bool Radler::IsInitialized() const {
  return parallel_deconvolution_->IsInitialized();
}

size_t Radler::IterationNumber() const {
  return parallel_deconvolution_->FirstAlgorithm().IterationNumber();
}

}  // namespace radler
