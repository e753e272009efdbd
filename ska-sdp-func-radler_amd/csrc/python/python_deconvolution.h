// radler::algorithms::PythonDeconvolution: a deconvolution algorithm written
// by the user as a Python function (AlgorithmType::kPython,
// Settings::Python::filename; the reference's
// cpp/algorithms/python_deconvolution.h). It is part of the `radler` Python
// module, not of libradler_amd: the host library links no libpython and gets
// the algorithm through python_deconvolution_factory.h.
//
// The file defines one of
//   deconvolve(residual, model, psf, meta)         numpy float64 copies on
//                                                   the host (the reference's
//                                                   contract)
//   deconvolve_device(residual, model, psf, meta)  radler.gpu.DeviceArray:
//                                                   float32 views of the image
//                                                   sets' own device memory,
//                                                   exchanged through DLPack
// DESIGN.md 4b states both contracts, and the lifetime and ordering rules of
// the device views.
#pragma once

#include <pybind11/pybind11.h>

#include <memory>
#include <string>
#include <vector>

#include "deconvolution_algorithm.h"

namespace radler::algorithms {

class PythonDeconvolution final : public DeconvolutionAlgorithm {
 public:
  /// Evaluates the file in a namespace of its own and takes its function.
  /// std::runtime_error with Python's message when that fails.
  explicit PythonDeconvolution(const std::string& filename);
  ~PythonDeconvolution() override;

  DeconvolutionResult ExecuteMajorIteration(ImageSet& data_image, ImageSet& model_image,
                                            const gpu::Planes& psf_images) override;
  /// The clones (a grid's subimages) share the loaded function.
  std::unique_ptr<DeconvolutionAlgorithm> Clone() const override;

 private:
  PythonDeconvolution(const PythonDeconvolution& other);

  std::string filename_;
  // An owned reference, held raw: the destructor decides whether the
  // interpreter is still there to give it back to.
  PyObject* function_ = nullptr;
  bool device_mode_ = false;
};

}  // namespace radler::algorithms

namespace radler::python {

/// Planes in the caller's device memory, imported over DLPack: what a
/// DeviceImageAccessor is made of. `keep_alive` owns the consumed
/// DLManagedTensor; its deleter runs when the last copy is released (with
/// the GIL, when the interpreter is still there to give it).
struct DeviceImages {
  std::shared_ptr<void> keep_alive;
  float* data = nullptr;
  std::vector<int64_t> shape;
  int device = 0;
};

/// An object that is not a numpy array and has __dlpack__: a candidate for
/// ImportDeviceImages.
bool IsDlpackObject(const pybind11::handle& object);

/// Consumes object.__dlpack__(). The tensor must be on a ROCm device, float32
/// and C-contiguous (byte_offset is honoured); pybind11::type_error naming
/// `argument` and the failed requirement otherwise. The shape is the caller's
/// to check.
DeviceImages ImportDeviceImages(const pybind11::object& object, const std::string& argument);

/// radler.gpu.DeviceArray and the radler.python_deconvolution helper classes
/// (Channel, MetaData, SpectralFitter), registered once; sets the host
/// library's factory. Needs the radler.gpu submodule to exist.
void InitPythonDeconvolution(pybind11::module_& m);

}  // namespace radler::python
