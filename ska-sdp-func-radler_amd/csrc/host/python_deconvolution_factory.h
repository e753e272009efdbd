// AlgorithmType::kPython without libpython in this library: the algorithm
// (csrc/python/python_deconvolution.cc) is part of the `radler` Python module,
// which registers its factory here when it is imported.
// Radler::InitializeDeconvolutionAlgorithm calls the factory; a process that
// never imported the module (a C++ host) has none, and gets an error saying
// so. Embedding an interpreter for such hosts is out of scope.
#pragma once

#include <memory>
#include <string>

#include "deconvolution_algorithm.h"

namespace radler::algorithms {

/// Makes the algorithm that runs the user's file `filename`
/// (Settings::Python::filename). Throws std::runtime_error when the file
/// cannot be loaded.
using PythonDeconvolutionFactory =
    std::unique_ptr<DeconvolutionAlgorithm> (*)(const std::string& filename);

/// Set once by the `radler` module at import (nullptr unregisters).
void SetPythonDeconvolutionFactory(PythonDeconvolutionFactory factory);

/// The registered factory's algorithm for `filename`; std::runtime_error when
/// no factory is registered.
std::unique_ptr<DeconvolutionAlgorithm> MakePythonDeconvolution(
    const std::string& filename);

}  // namespace radler::algorithms
