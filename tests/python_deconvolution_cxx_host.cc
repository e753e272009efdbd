// A C++ host that links libradler_amd.so and never loads the radler Python
// module asks for AlgorithmType::kPython: no factory is registered
// (csrc/host/python_deconvolution_factory.h), so the Radler constructor throws
// a std::runtime_error that says what is missing. Prints the message;
// tests/test_python_deconvolution.py checks it. Needs no device.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "radler.h"

int main() {
  const size_t width = 40, height = 24;
  radler::Settings settings;
  settings.algorithm_type = radler::AlgorithmType::kPython;
  settings.python.filename = "never_opened.py";
  settings.trimmed_image_width = width;
  settings.trimmed_image_height = height;
  settings.pixel_scale.x = settings.pixel_scale.y = 1.0e-4;
  std::vector<float> psf(width * height, 0.0f), residual(psf), model(psf);
  aocommon::Image psf_image(psf.data(), width, height);
  aocommon::Image residual_image(residual.data(), width, height);
  aocommon::Image model_image(model.data(), width, height);
  try {
    radler::Radler radler(settings, psf_image, residual_image, model_image, 0.0);
  } catch (const std::runtime_error& e) {
    std::printf("%s\n", e.what());
    return 0;
  }
  std::printf("no exception\n");
  return 1;
}
