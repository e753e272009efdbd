// A C++ host of libradler_amd.so whose images live in device memory
// (radler::utils::DeviceImageAccessor, the DeviceImage constructor of Radler).
//
//   device_accessor_cxx_host cpu   what needs no device: the accessor's
//                                  properties and the checks made when a Radler
//                                  is constructed
//   device_accessor_cxx_host gpu   two channels in one deconvolution group,
//                                  allocated with rdl_malloc, cleaned through a
//                                  work table of DeviceImageAccessors and, from
//                                  the same data, through
//                                  LoadAndStoreImageAccessors over host images:
//                                  flags, iteration numbers and every bit of
//                                  residual and model must agree, the PSFs stay
//                                  as they were; then the single-image
//                                  constructor the same way
// Prints OK and returns 0; a message and 1 otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "device.h"
#include "image_accessors.h"
#include "radler.h"

namespace {

constexpr size_t kWidth = 64, kHeight = 48, kPixels = kWidth * kHeight;

using radler::utils::DeviceImageAccessor;

[[noreturn]] void Fail(const std::string& what) { throw std::runtime_error(what); }

radler::Settings MakeSettings() {
  radler::Settings settings;
  settings.algorithm_type = radler::AlgorithmType::kGenericClean;
  settings.trimmed_image_width = kWidth;
  settings.trimmed_image_height = kHeight;
  settings.pixel_scale.x = settings.pixel_scale.y = 1.0e-4;
  settings.minor_iteration_count = 80;
  settings.absolute_threshold = 1.0e-3;
  settings.major_loop_gain = 0.7;
  return settings;
}

/// `make()` must throw a std::runtime_error whose text has every word.
void ExpectError(const char* what, const std::function<void()>& make,
                 const std::vector<std::string>& words) {
  try {
    make();
  } catch (const std::runtime_error& e) {
    for (const std::string& word : words)
      if (std::string(e.what()).find(word) == std::string::npos)
        Fail(std::string(what) + ": message '" + e.what() + "' lacks '" + word + "'");
    return;
  }
  Fail(std::string(what) + ": no std::runtime_error");
}

std::unique_ptr<radler::WorkTable> OneEntryTable(float* psf, float* residual, float* model,
                                                 size_t width, size_t height, int device,
                                                 bool residual_writable) {
  auto table = std::make_unique<radler::WorkTable>(std::vector<radler::PsfOffset>{}, 1, 1);
  auto e = std::make_unique<radler::WorkTableEntry>();
  e->image_weight = 1.0;
  e->psf_accessors.emplace_back(
      std::make_unique<DeviceImageAccessor>(psf, width, height, device, false));
  e->residual_accessor =
      std::make_unique<DeviceImageAccessor>(residual, width, height, device, residual_writable);
  e->model_accessor = std::make_unique<DeviceImageAccessor>(model, width, height, device, true);
  table->AddEntry(std::move(e));
  return table;
}

int Cpu() {
  // addresses only: nothing here touches the device
  float* base = reinterpret_cast<float*>(uintptr_t(1) << 32);
  DeviceImageAccessor read_only(base, 40, 24, 3, false);
  if (read_only.Width() != 40 || read_only.Height() != 24 || read_only.Device() != 3 ||
      read_only.Writable() || read_only.Data() != base ||
      read_only.Bytes() != 40 * 24 * sizeof(float))
    Fail("DeviceImageAccessor does not report what it was made with");
  if (!DeviceImageAccessor(base, 1, 1, 0, true).Writable()) Fail("writable flag lost");
  const aocommon::ImageAccessor& generic = read_only;
  if (generic.Width() != 40 || generic.Height() != 24) Fail("ImageAccessor view differs");
  try {
    std::vector<float> host(40 * 24);
    read_only.Store(host.data());
    Fail("Store() on a read-only accessor did not throw");
  } catch (const std::logic_error&) {
  }
  {
    auto keep = std::make_shared<int>(7);
    std::weak_ptr<int> watch = keep;
    {
      DeviceImageAccessor owner(base, 1, 1, 0, true, std::move(keep));
      if (watch.expired()) Fail("keep-alive released early");
    }
    if (!watch.expired()) Fail("keep-alive not released with the accessor");
  }

  const radler::Settings settings = MakeSettings();
  float* psf = base;
  float* residual = base + kPixels;
  float* model = base + 2 * kPixels;
  // a valid table constructs without a device
  radler::Radler(settings, OneEntryTable(psf, residual, model, kWidth, kHeight, 0, true), 0.0);
  ExpectError("read-only residual", [&] {
    radler::Radler(settings, OneEntryTable(psf, residual, model, kWidth, kHeight, 0, false), 0.0);
  }, {"residual image of entry 0", "read-only"});
  ExpectError("other device", [&] {
    radler::Radler(settings, OneEntryTable(psf, residual, model, kWidth, kHeight, 5, true), 0.0);
  }, {"of entry 0", "device 5", "device 0"});
  ExpectError("size", [&] {
    radler::Radler(settings, OneEntryTable(psf, residual, model, kWidth, kHeight - 1, 0, true),
                   0.0);
  }, {"residual image of entry 0", "64 x 47", "64 x 48"});
  ExpectError("overlap", [&] {
    radler::Radler(settings, OneEntryTable(psf, residual, residual + 5, kWidth, kHeight, 0, true),
                   0.0);
  }, {"residual image of entry 0", "overlaps", "model image of entry 0"});
  ExpectError("constructor size", [&] {
    radler::DeviceImage image{psf, kWidth, kHeight, 0}, small{residual, kWidth, kHeight - 1, 0};
    radler::Radler(settings, image, small, radler::DeviceImage{model, kWidth, kHeight, 0}, 0.0);
  }, {"Mismatch in residual image size"});
  return 0;
}

void MakeImages(size_t n_channels, std::vector<float>& psf, std::vector<float>& residual) {
  psf.assign(n_channels * kPixels, 0.0f);
  residual.assign(n_channels * kPixels, 0.0f);
  for (size_t c = 0; c != n_channels; ++c) {
    float* p = psf.data() + c * kPixels;
    const double sigma = 1.5 + 0.3 * double(c);
    for (size_t y = 0; y != kHeight; ++y)
      for (size_t x = 0; x != kWidth; ++x) {
        const double dx = double(x) - kWidth / 2, dy = double(y) - kHeight / 2;
        p[y * kWidth + x] = float(std::exp(-0.5 * (dx * dx + dy * dy) / (sigma * sigma)));
      }
    // three sources, each the PSF shifted and scaled
    const int sources[3][3] = {{-12, 5, 100}, {9, -8, 60}, {3, 14, 35}};
    float* r = residual.data() + c * kPixels;
    for (const auto& source : sources)
      for (size_t y = 0; y != kHeight; ++y)
        for (size_t x = 0; x != kWidth; ++x) {
          const long sx = long(x) - source[0], sy = long(y) - source[1];
          if (sx < 0 || sy < 0 || sx >= long(kWidth) || sy >= long(kHeight)) continue;
          r[y * kWidth + x] += 0.01f * float(source[2]) * (1.0f + 0.1f * float(c)) *
                               p[size_t(sy) * kWidth + size_t(sx)];
        }
  }
}

struct Outcome {
  std::vector<bool> flags;
  std::vector<size_t> iterations;
};

Outcome Run(radler::Radler& radler) {
  Outcome out;
  for (size_t major = 1; major <= 2; ++major) {
    bool another = false;
    radler.Perform(another, major);
    out.flags.push_back(another);
    out.iterations.push_back(radler.IterationNumber());
  }
  return out;
}

void Compare(const char* what, radler::gpu::Session& session, const Outcome& host_run,
             const Outcome& device_run, const std::vector<float>& psf,
             const std::vector<float>& residual, const std::vector<float>& model,
             const float* d_psf, const float* d_residual, const float* d_model) {
  if (host_run.flags != device_run.flags || host_run.iterations != device_run.iterations)
    Fail(std::string(what) + ": flags or iteration numbers differ");
  if (host_run.iterations.back() == 0) Fail(std::string(what) + ": nothing was cleaned");
  std::vector<float> back(psf.size());
  const auto same = [&](const float* d_plane, const std::vector<float>& host, const char* name) {
    session.D2H(back.data(), d_plane, back.size() * sizeof(float));
    session.Sync();
    if (std::memcmp(back.data(), host.data(), back.size() * sizeof(float)) != 0)
      Fail(std::string(what) + ": " + name + " differs from the host-accessor run");
  };
  same(d_psf, psf, "psf");
  same(d_residual, residual, "residual");
  same(d_model, model, "model");
}

int Gpu() {
  const std::shared_ptr<radler::gpu::Session> session = radler::gpu::Session::ForDevice(0);
  rdl_session* s = session->Handle();
  for (const size_t n_channels : {size_t(2), size_t(1)}) {
    const char* what = n_channels == 2 ? "work table" : "DeviceImage constructor";
    std::vector<float> psf, residual;
    MakeImages(n_channels, psf, residual);
    const std::vector<float> psf_before = psf;
    std::vector<float> model(psf.size(), 0.0f);
    const size_t bytes = psf.size() * sizeof(float);
    void* allocations[3] = {nullptr, nullptr, nullptr};
    for (void*& allocation : allocations)
      radler::gpu::Check(rdl_malloc(s, bytes, &allocation), "rdl_malloc");
    float* d_psf = static_cast<float*>(allocations[0]);
    float* d_residual = static_cast<float*>(allocations[1]);
    float* d_model = static_cast<float*>(allocations[2]);
    session->H2D(d_psf, psf.data(), bytes);
    session->H2D(d_residual, residual.data(), bytes);
    session->H2D(d_model, model.data(), bytes);
    session->Sync();

    const radler::Settings settings = MakeSettings();
    std::unique_ptr<radler::Radler> host_radler, device_radler;
    if (n_channels == 1) {
      aocommon::Image psf_image(psf.data(), kWidth, kHeight);
      aocommon::Image residual_image(residual.data(), kWidth, kHeight);
      aocommon::Image model_image(model.data(), kWidth, kHeight);
      host_radler = std::make_unique<radler::Radler>(settings, psf_image, residual_image,
                                                     model_image, 0.0);
      device_radler = std::make_unique<radler::Radler>(
          settings, radler::DeviceImage{d_psf, kWidth, kHeight, 0},
          radler::DeviceImage{d_residual, kWidth, kHeight, 0},
          radler::DeviceImage{d_model, kWidth, kHeight, 0}, 0.0);
    } else {
      auto host_table =
          std::make_unique<radler::WorkTable>(std::vector<radler::PsfOffset>{}, n_channels, 1);
      auto device_table =
          std::make_unique<radler::WorkTable>(std::vector<radler::PsfOffset>{}, n_channels, 1);
      for (size_t c = 0; c != n_channels; ++c) {
        const size_t at = c * kPixels;
        for (const bool on_device : {false, true}) {
          auto e = std::make_unique<radler::WorkTableEntry>();
          e->original_channel_index = c;
          e->band_start_frequency = 100.0e6 + 10.0e6 * double(c);
          e->band_end_frequency = e->band_start_frequency + 10.0e6;
          e->image_weight = 1.0 + 0.5 * double(c);
          if (on_device) {
            e->psf_accessors.emplace_back(
                std::make_unique<DeviceImageAccessor>(d_psf + at, kWidth, kHeight, 0, false));
            e->residual_accessor =
                std::make_unique<DeviceImageAccessor>(d_residual + at, kWidth, kHeight, 0, true);
            e->model_accessor =
                std::make_unique<DeviceImageAccessor>(d_model + at, kWidth, kHeight, 0, true);
            device_table->AddEntry(std::move(e));
          } else {
            aocommon::Image psf_image(psf.data() + at, kWidth, kHeight);
            aocommon::Image residual_image(residual.data() + at, kWidth, kHeight);
            aocommon::Image model_image(model.data() + at, kWidth, kHeight);
            e->psf_accessors.emplace_back(
                std::make_unique<radler::utils::LoadOnlyImageAccessor>(psf_image));
            e->residual_accessor =
                std::make_unique<radler::utils::LoadAndStoreImageAccessor>(residual_image);
            e->model_accessor =
                std::make_unique<radler::utils::LoadAndStoreImageAccessor>(model_image);
            host_table->AddEntry(std::move(e));
          }
        }
      }
      host_radler = std::make_unique<radler::Radler>(settings, std::move(host_table), 0.0);
      device_radler = std::make_unique<radler::Radler>(settings, std::move(device_table), 0.0);
    }
    const Outcome host_run = Run(*host_radler);
    const Outcome device_run = Run(*device_radler);
    if (psf != psf_before) Fail("the host run changed its PSF");
    Compare(what, *session, host_run, device_run, psf, residual, model, d_psf, d_residual,
            d_model);
    // the generic accessor interface still works on device memory
    DeviceImageAccessor generic(d_model, kWidth, kHeight, 0, true);
    std::vector<float> loaded(kPixels);
    generic.Load(loaded.data());
    if (std::memcmp(loaded.data(), model.data(), kPixels * sizeof(float)) != 0)
      Fail("DeviceImageAccessor::Load differs from the model");
    loaded[7] = 42.0f;
    generic.Store(loaded.data());
    std::vector<float> again(kPixels);
    generic.Load(again.data());
    if (again != loaded) Fail("DeviceImageAccessor::Store / Load round trip");
    device_radler.reset();
    host_radler.reset();
    for (void* allocation : allocations) radler::gpu::Check(rdl_free(s, allocation), "rdl_free");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "cpu")
      Cpu();
    else if (mode == "gpu")
      Gpu();
    else
      Fail("usage: device_accessor_cxx_host cpu|gpu");
  } catch (const std::exception& e) {
    std::printf("FAILED: %s\n", e.what());
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
