#include "device_image_accessor.h"

#include <stdexcept>

#include "device.h"

namespace radler::utils {

// The generic path: code that knows nothing of device accessors. The copies
// run on the device's process-wide session; the device is synchronised first
// because the plane's producer may have used any stream.
void DeviceImageAccessor::Load(float* data) const {
  const std::shared_ptr<gpu::Session> session = gpu::Session::ForDevice(device_);
  session->DeviceSync();
  session->D2H(data, data_, Bytes());
  session->Sync();
}

void DeviceImageAccessor::Store(const float* data) {
  if (!writable_)
    throw std::logic_error("DeviceImageAccessor::Store() on a read-only device image");
  const std::shared_ptr<gpu::Session> session = gpu::Session::ForDevice(device_);
  session->DeviceSync();
  session->H2D(data_, data, Bytes());
  session->Sync();
}

}  // namespace radler::utils
