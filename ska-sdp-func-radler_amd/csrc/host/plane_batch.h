// radler::PlaneBatch — many independent planes of one size, each cleaned as a
// Radler of its own would clean it (algorithm_type = kGenericClean,
// generic.use_sub_minor_optimization = false), all of them in one persistent
// launch per Perform (rdl_hogbom_batch_run). The reference joins
// everything in a WorkTable, so it has no counterpart there: the channels of a
// spectral-line cube cleaned without joining, snapshot images per time slice,
// cut-outs around catalogue positions.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "aocommon_compat.h"
#include "device_image_accessor.h"
#include "settings.h"

namespace radler {
namespace gpu {
class Buffer;
class Session;
}  // namespace gpu

class PlaneBatch {
 public:
  /// Planes of width x height floats each, all on the host or all in the
  /// memory of HIP device `device` (there at one constant distance of at
  /// least a plane from each other, as the planes of a stack are).
  /// `keep_alive` (optional) owns the memory.
  struct Planes {
    std::vector<float*> planes;
    bool on_device = false;
    int device = 0;
    std::shared_ptr<void> keep_alive;
  };

  /// `psfs`: one plane for every item, or one per item. `masks`: none, one
  /// or one per item, host planes of width x height bytes (non-zero: the
  /// pixel may hold a component), copied here. Residuals and models are both
  /// host planes or both device planes; they are read and written in place
  /// by Perform and stay valid while this object is used. Every setting this
  /// class does not honour raises std::runtime_error naming it, before any
  /// device is touched.
  PlaneBatch(const Settings& settings, Planes psfs, Planes residuals, Planes models,
             const std::vector<const uint8_t*>& masks = {});
  /// Host images.
  PlaneBatch(const Settings& settings, const std::vector<aocommon::Image>& psfs,
             std::vector<aocommon::Image>& residuals, std::vector<aocommon::Image>& models,
             const std::vector<const uint8_t*>& masks = {});
  /// Planes that already live in device memory, read and written in place.
  PlaneBatch(const Settings& settings, const std::vector<DeviceImage>& psfs,
             const std::vector<DeviceImage>& residuals, const std::vector<DeviceImage>& models,
             const std::vector<const uint8_t*>& masks = {});
  ~PlaneBatch();

  /// Plane b's Radler::Perform. The first call cleans every plane, each later
  /// one the planes whose flag the call before left true; the flags of the
  /// others come back false.
  void Perform(std::vector<bool>& another_iteration_required, size_t major_iteration_number);
  /// Radler::IterationNumber per plane, accumulated over the calls.
  const std::vector<size_t>& IterationNumbers() const { return iterations_; }
  size_t NPlanes() const { return residuals_.planes.size(); }

 private:
  void Validate(size_t n_masks) const;
  int DeviceIndex() const;

  const Settings settings_;
  size_t width_, height_;
  Planes psfs_, residuals_, models_;
  std::vector<uint8_t> masks_;  // n_masks_ planes
  size_t n_masks_ = 0;
  std::vector<size_t> iterations_;
  std::vector<bool> required_;
  bool performed_ = false;
  std::shared_ptr<gpu::Session> session_;
  // device copies of what came from the host, and of the masks
  std::unique_ptr<gpu::Buffer> d_psfs_, d_residuals_, d_models_, d_masks_;
};

}  // namespace radler
