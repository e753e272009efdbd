// radler::Radler — the public entry point (reference: cpp/radler.{h,cc}),
// same constructors, Perform() contract and accessors. Image data is
// uploaded to the GPU after ImageSet::LoadAndAverage and written back through
// the WorkTable accessors at the end of Perform(), as the reference's
// residual/model stores do.
#pragma once

#include <memory>

#include "aocommon_compat.h"
#include "component_list.h"
#include "device_image_accessor.h"
#include "settings.h"
#include "spectral_fitter.h"
#include "work_table.h"
#include "work_table_entry.h"

namespace radler {
namespace algorithms {
class ParallelDeconvolution;
class DeconvolutionAlgorithm;
}  // namespace algorithms
namespace gpu {
class Session;
}
class Communicator;

class Radler {
 public:
  Radler(const Settings& settings, std::unique_ptr<WorkTable> table,
         double beam_size);
  /// Single channel, single polarization (radler.h:42-46). Keep the image
  /// buffers alive while this object is used.
  Radler(const Settings& settings, const aocommon::Image& psf_image,
         aocommon::Image& residual_image, aocommon::Image& model_image,
         double beam_size,
         aocommon::PolarizationEnum polarization =
             aocommon::PolarizationEnum::StokesI);
  /// The same for images that already live in device memory: the PSF is read
  /// and residual and model are read and written where they are, with no
  /// copy through the host. The planes stay valid, and are not written by
  /// anyone else during Perform(), while this object is used.
  Radler(const Settings& settings, const DeviceImage& psf_image,
         const DeviceImage& residual_image, const DeviceImage& model_image,
         double beam_size,
         aocommon::PolarizationEnum polarization =
             aocommon::PolarizationEnum::StokesI);
  ~Radler();

  ComponentList GetComponentList() const;
  const algorithms::DeconvolutionAlgorithm& MaxScaleCountAlgorithm() const;
  void Perform(bool& another_iteration_required, size_t major_iteration_number);
  void FreeDeconvolutionAlgorithms();
  std::unique_ptr<schaapcommon::fitters::SpectralFitter> CreateSpectralFitter()
      const;
  bool IsInitialized() const;
  size_t IterationNumber() const;
  /// Perform has left the auto-mask tracking phase: the masks are now used.
  bool AutoMaskIsFinished() const { return auto_mask_is_finished_; }

  // MI355X build only: the device session (bench / tests) and the
  // parallel-deconvolution object.
  gpu::Session& DeviceSession() const;
  /// The settings this Radler was made with (ComponentList::Render takes the
  /// multiscale shape from them).
  const Settings& GetSettings() const { return settings_; }
  algorithms::ParallelDeconvolution& Parallel() const {
    return *parallel_deconvolution_;
  }
  /// MI355X build: share the subimages of gridded runs (settings.parallel
  /// grid > 1x1) with the other ranks of a process-per-GPU job; every rank
  /// calls Perform with the same inputs and gets the same result.
  void SetCommunicator(std::shared_ptr<Communicator> comm);

 private:
  Radler(const Settings& settings, double beam_size);
  void InitializeDeconvolutionAlgorithm(std::unique_ptr<WorkTable> table);
  /// The device accessors of the table against the session's device, the
  /// image size, writability and each other; std::runtime_error.
  void ValidateDeviceImages() const;
  int DeviceIndex() const;
  /// radler.cc:410-432: the term cube of settings.spectral_fitting.forced_filename
  void ReadForcedSpectrumImages();
  /// radler.cc:434-527: settings.fits_mask and the horizon mask
  void ReadMask(const WorkTable& group_table);

  const Settings settings_;
  std::unique_ptr<WorkTable> table_;
  bool has_device_images_ = false;  // any DeviceImageAccessor in table_
  mutable std::shared_ptr<gpu::Session> session_;
  std::unique_ptr<algorithms::ParallelDeconvolution> parallel_deconvolution_;
  size_t image_width_ = 0;
  size_t image_height_ = 0;
  double pixel_scale_x_ = 0.0;
  double pixel_scale_y_ = 0.0;
  double beam_size_ = 0.0;
  // auto-masking state across major iterations (cpp/radler.h:111-114)
  bool auto_mask_is_finished_ = false;
  size_t auto_mask_finishing_iteration_ = 0;
  std::vector<uint8_t> auto_mask_;  // scale-independent mask (non-multiscale)
  std::vector<uint8_t> clean_mask_;  // fits / horizon mask (bool as bytes)
  std::vector<float> rms_file_image_;  // settings.local_rms.image, read once
};

}  // namespace radler
