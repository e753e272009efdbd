// An accessor over a plane that already lives in device memory (a GPU
// gridder's output, a torch tensor, the planes of an earlier Radler run).
// ImageSet recognises it (dynamic_cast) and reads and writes the plane where
// it is; to every other caller it is an ordinary aocommon::ImageAccessor
// whose Load / Store copy through the host.
#pragma once

#include <cstddef>
#include <memory>

#include "aocommon_compat.h"

namespace radler {

/// A width x height float plane in the memory of HIP device `device`: what
/// the device-pointer constructor of Radler takes.
struct DeviceImage {
  float* data = nullptr;
  size_t width = 0, height = 0;
  int device = 0;
};

}  // namespace radler

namespace radler::utils {

class DeviceImageAccessor final : public aocommon::ImageAccessor {
 public:
  /// `d_data`: width * height floats, row-major, on HIP device `device`,
  /// 4-byte aligned. `keep_alive` (optional) owns the memory: it is released
  /// when the accessor is destroyed. Without it the caller keeps the memory
  /// valid for as long as the work table lives.
  DeviceImageAccessor(float* d_data, size_t width, size_t height, int device, bool writable,
                      std::shared_ptr<void> keep_alive = nullptr)
      : data_(d_data),
        width_(width),
        height_(height),
        device_(device),
        writable_(writable),
        keep_alive_(std::move(keep_alive)) {}

  size_t Width() const override { return width_; }
  size_t Height() const override { return height_; }
  /// Blocking copy of the plane to `data` (host).
  void Load(float* data) const override;
  /// Blocking copy of `data` (host) to the plane; std::logic_error when the
  /// accessor is not writable.
  void Store(const float* data) override;

  float* Data() const { return data_; }
  int Device() const { return device_; }
  bool Writable() const { return writable_; }
  size_t Bytes() const { return width_ * height_ * sizeof(float); }

 private:
  float* data_;
  size_t width_, height_;
  int device_;
  bool writable_;
  std::shared_ptr<void> keep_alive_;
};

}  // namespace radler::utils
