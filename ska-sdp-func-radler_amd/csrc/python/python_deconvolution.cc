// See python_deconvolution.h. Written from the behaviour of the reference's
// cpp/algorithms/python_deconvolution.cc (the contract of deconvolve(), its
// meta data and its error messages' prefixes); the device contract is this
// build's own.
//
// GIL: every function here that touches a Python object holds the GIL for as
// long as it does, and turns a Python error into a std::runtime_error before
// the GIL is given back, so no pybind11::error_already_set (which owns Python
// references) leaves such a scope. Radler.perform runs with the GIL released;
// ExecuteMajorIteration takes it for the call and gives it back around every
// wait for the device. ParallelDeconvolution calls ExecuteMajorIteration with
// none of its mutexes held (DeconvolveSubImage), so the pool's workers simply
// take the GIL in turn.
#include "python_deconvolution.h"

#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <fstream>
#include <iterator>
#include <sstream>
#include <stdexcept>
#include <vector>

#include "dlpack_abi.h"
#include "python_deconvolution_factory.h"

namespace py = pybind11;
using schaapcommon::fitters::SpectralFitter;
using schaapcommon::fitters::SpectralFittingMode;

namespace radler::python {
namespace {

constexpr const char* kCallErrorPrefix =
    "Error occurred while executing python deconvolution function: ";
constexpr const char* kResultErrorPrefix = "In python deconvolution code: ";

// ---------------------------------------------------------------- meta data
struct PyChannel {
  double frequency = 0.0, weight = 0.0;
};

/// meta.spectral_fitter: the algorithm's fitter for one component's values.
class PySpectralFitter {
 public:
  explicit PySpectralFitter(std::shared_ptr<const SpectralFitter> fitter)
      : fitter_(std::move(fitter)) {}

  py::array_t<double> Fit(const py::object& values, size_t x, size_t y) const {
    if (fitter_->Mode() == SpectralFittingMode::kNoFitting)
      throw std::runtime_error("spectral_fitter.fit: no spectral fitting mode is selected");
    const std::vector<float> channel_values = Values(values, "spectral_fitter.fit");
    std::vector<float> terms;
    fitter_->Fit(terms, channel_values.data(), x, y);
    terms.resize(fitter_->NTerms());
    return ToArray(terms);
  }

  py::object FitAndEvaluate(const py::object& values, size_t x, size_t y) const {
    if (fitter_->Mode() == SpectralFittingMode::kNoFitting) return values;
    std::vector<float> channel_values = Values(values, "spectral_fitter.fit_and_evaluate");
    std::vector<float> scratch;
    fitter_->FitAndEvaluate(channel_values.data(), x, y, scratch);
    return ToArray(channel_values);
  }

 private:
  std::vector<float> Values(const py::object& values, const char* who) const {
    auto array = py::array_t<double, py::array::forcecast>::ensure(values);
    if (!array) {
      PyErr_Clear();
      throw std::runtime_error(std::string(who) + ": values cannot be read as a float array");
    }
    const size_t needed = fitter_->Frequencies().size();
    if (array.ndim() != 1)
      throw std::runtime_error(std::string(who) + ": values has " +
                               std::to_string(array.ndim()) +
                               " dimensions, a 1-D array of one value per channel is needed");
    if (size_t(array.shape(0)) != needed)
      throw std::runtime_error(std::string(who) + ": values has the wrong length (got " +
                               std::to_string(array.shape(0)) + ", need " +
                               std::to_string(needed) + ", one per channel)");
    std::vector<float> out(needed);
    auto view = array.unchecked<1>();
    for (size_t i = 0; i != needed; ++i) out[i] = float(view(py::ssize_t(i)));
    return out;
  }

  static py::array_t<double> ToArray(const std::vector<float>& v) {
    const py::ssize_t n = py::ssize_t(v.size());
    py::array_t<double> out(n);
    std::copy(v.begin(), v.end(), out.mutable_data());
    return out;
  }

  std::shared_ptr<const SpectralFitter> fitter_;
};

struct PyMetaData {
  explicit PyMetaData(std::shared_ptr<const SpectralFitter> fitter)
      : spectral_fitter(std::move(fitter)) {}
  std::vector<PyChannel> channels;
  size_t iteration_number = 0;
  double final_threshold = 0.0;
  double gain = 0.0;
  size_t max_iterations = 0;
  double major_iter_threshold = 0.0;
  double mgain = 0.0;
  PySpectralFitter spectral_fitter;
  bool square_joined_channels = false;
};

// -------------------------------------------------------------- DeviceArray
/// A float32, C-contiguous view of device memory that an image set (or a PSF
/// stack) owns. The view, and every DLPack capsule made from it, holds the
/// allocation: what outlives the call reads stale memory, never freed memory.
struct DeviceArray {
  std::shared_ptr<gpu::Buffer> buffer;
  float* data = nullptr;
  std::vector<int64_t> shape;
  int device = 0;
};

struct ExportContext {
  DLManagedTensor tensor;
  std::shared_ptr<gpu::Buffer> keep;
  std::vector<int64_t> shape, strides;
};

void DeleteExport(DLManagedTensor* self) { delete static_cast<ExportContext*>(self->manager_ctx); }

// A capsule nobody consumed still owns its tensor (a consumer renames it).
void DestroyCapsule(PyObject* capsule) {
  if (!PyCapsule_IsValid(capsule, "dltensor")) return;
  auto* tensor = static_cast<DLManagedTensor*>(PyCapsule_GetPointer(capsule, "dltensor"));
  if (tensor && tensor->deleter) tensor->deleter(tensor);
}

std::vector<int64_t> CompactStrides(const std::vector<int64_t>& shape) {
  std::vector<int64_t> strides(shape.size(), 1);
  for (size_t i = shape.size(); i-- > 1;) strides[i - 1] = strides[i] * shape[i];
  return strides;
}

py::object ExportDlpack(const DeviceArray& array) {
  auto context = std::make_unique<ExportContext>();
  context->keep = array.buffer;
  context->shape = array.shape;
  context->strides = CompactStrides(array.shape);
  DLManagedTensor& t = context->tensor;
  t.dl_tensor.data = array.data;
  t.dl_tensor.device.device_type = kDLROCM;
  t.dl_tensor.device.device_id = array.device;
  t.dl_tensor.ndim = int32_t(context->shape.size());
  t.dl_tensor.dtype.code = kDLFloat;
  t.dl_tensor.dtype.bits = 32;
  t.dl_tensor.dtype.lanes = 1;
  t.dl_tensor.shape = context->shape.data();
  t.dl_tensor.strides = context->strides.data();
  t.dl_tensor.byte_offset = 0;
  t.manager_ctx = context.get();
  t.deleter = DeleteExport;
  PyObject* capsule = PyCapsule_New(&t, "dltensor", DestroyCapsule);
  if (!capsule) throw py::error_already_set();
  context.release();  // the capsule's, then its consumer's
  return py::reinterpret_steal<py::object>(capsule);
}

std::string ShapeText(const int64_t* shape, size_t n) {
  std::ostringstream s;
  s << '(';
  for (size_t i = 0; i != n; ++i) s << (i ? ", " : "") << shape[i];
  s << ')';
  return s.str();
}
std::string ShapeText(const std::vector<int64_t>& shape) {
  return ShapeText(shape.data(), shape.size());
}

std::string TypeName(const py::handle& object) { return Py_TYPE(object.ptr())->tp_name; }

[[noreturn]] void BadResult(const std::string& what) {
  throw std::runtime_error(kResultErrorPrefix + what);
}

// ------------------------------------------------------------------ the call
struct CallShape {
  size_t n_freq, n_pol, height, width;
  std::vector<int64_t> Images() const {
    return {int64_t(n_freq), int64_t(n_pol), int64_t(height), int64_t(width)};
  }
  std::vector<int64_t> Psfs() const {
    return {int64_t(n_freq), int64_t(height), int64_t(width)};
  }
};

size_t Count(const std::vector<int64_t>& shape) {
  size_t n = 1;
  for (int64_t d : shape) n *= size_t(d);
  return n;
}

/// float32 device planes as a new float64 numpy array (rdl_convert, then one
/// copy to the host). The GIL is given back while the device is waited for.
py::array_t<double> ToHost(gpu::Session& s, const float* d_planes,
                           const std::vector<int64_t>& shape) {
  py::array_t<double> array(std::vector<py::ssize_t>(shape.begin(), shape.end()));
  double* h_dst = array.mutable_data();
  const size_t n = Count(shape);
  {
    py::gil_scoped_release release;
    gpu::Buffer d_f64(s, n * sizeof(double));
    gpu::Check(rdl_convert(s.Handle(), d_planes, d_f64.Ptr(), n, 1), "rdl_convert");
    s.D2H(h_dst, d_f64.Ptr(), n * sizeof(double));
  }
  return array;
}

/// `object` as a C-contiguous float64 array of exactly `shape`.
py::array_t<double> HostResult(const py::handle& object, const char* key,
                               const std::vector<int64_t>& shape) {
  auto array =
      py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(object);
  if (!array) {
    PyErr_Clear();
    BadResult("'" + std::string(key) + "' returned by deconvolve() is a " + TypeName(object) +
              ", which cannot be read as a float array");
  }
  std::vector<int64_t> got(array.shape(), array.shape() + array.ndim());
  if (got != shape)
    BadResult("'" + std::string(key) + "' returned by deconvolve() has shape " +
              ShapeText(got) + ", the image set has " + ShapeText(shape));
  return array;
}

void FromHost(gpu::Session& s, float* d_planes, const py::array_t<double>& array) {
  const double* h_src = array.data();
  const size_t n = size_t(array.size());
  py::gil_scoped_release release;
  gpu::Buffer d_f64(s, n * sizeof(double));
  s.H2D(d_f64.Ptr(), h_src, n * sizeof(double));
  gpu::Check(rdl_convert(s.Handle(), d_f64.Ptr(), d_planes, n, 0), "rdl_convert");
  s.Sync();
}

/// A device-mode `residual` / `model` that is neither absent, None nor the
/// view that was passed: validated as float32, C-contiguous, on the session's
/// device and of the set's shape, then copied device to device.
void CopyFromDlpack(gpu::Session& s, float* d_planes, const py::handle& object,
                    const char* key, const std::vector<int64_t>& shape) {
  const std::string name = "'" + std::string(key) + "' returned by deconvolve_device()";
  if (!py::hasattr(object, "__dlpack__"))
    BadResult(name + " is a " + TypeName(object) +
              ": it must be absent, None, the array that was passed, or an object with "
              "__dlpack__");
  py::object capsule = object.attr("__dlpack__")();
  if (!PyCapsule_IsValid(capsule.ptr(), "dltensor"))
    BadResult(name + ": its __dlpack__() did not return a 'dltensor' capsule");
  auto* managed =
      static_cast<DLManagedTensor*>(PyCapsule_GetPointer(capsule.ptr(), "dltensor"));
  const DLTensor& t = managed->dl_tensor;
  // (an invalid capsule is still its producer's: its destructor releases it)
  if (t.device.device_type != kDLROCM || t.device.device_id != s.Device())
    BadResult(name + " is on DLPack device (" + std::to_string(int(t.device.device_type)) +
              ", " + std::to_string(t.device.device_id) + "), not on ROCm device " +
              std::to_string(s.Device()) + " (" + std::to_string(int(kDLROCM)) + ", " +
              std::to_string(s.Device()) + ") of the image set");
  if (t.dtype.code != kDLFloat || t.dtype.bits != 32 || t.dtype.lanes != 1)
    BadResult(name + " has dtype (code " + std::to_string(int(t.dtype.code)) + ", " +
              std::to_string(int(t.dtype.bits)) + " bits), float32 is required");
  if (t.ndim != int32_t(shape.size()) || !std::equal(shape.begin(), shape.end(), t.shape))
    BadResult(name + " has shape " + ShapeText(t.shape, size_t(std::max(t.ndim, 0))) +
              ", the image set has " + ShapeText(shape));
  if (t.strides) {
    const std::vector<int64_t> compact = CompactStrides(shape);
    for (size_t i = 0; i != shape.size(); ++i)
      if (shape[i] > 1 && t.strides[i] != compact[i])
        BadResult(name + " is not C-contiguous (strides " +
                  ShapeText(t.strides, shape.size()) + " elements)");
  }
  // consumed from here on: the tensor is ours to delete
  PyCapsule_SetName(capsule.ptr(), "used_dltensor");
  struct Release {
    DLManagedTensor* tensor;
    ~Release() {
      if (tensor->deleter) tensor->deleter(tensor);
    }
  } release_tensor{managed};
  const char* d_src = static_cast<const char*>(t.data) + t.byte_offset;
  const size_t bytes = Count(shape) * sizeof(float);
  if (d_src == reinterpret_cast<const char*>(d_planes)) return;  // another view of the set
  py::gil_scoped_release release;
  s.D2D(d_planes, d_src, bytes);
  s.Sync();  // before the source can be freed
}

std::shared_ptr<PyMetaData> MakeMeta(const algorithms::DeconvolutionAlgorithm& algorithm,
                                     const ImageSet& data_image) {
  std::shared_ptr<const SpectralFitter> fitter = algorithm.SharedFitter();
  if (!fitter) fitter = std::make_shared<SpectralFitter>(SpectralFittingMode::kNoFitting, 0);
  auto meta = std::make_shared<PyMetaData>(fitter);
  const std::vector<double>& frequencies = fitter->Frequencies();
  const std::vector<float>& weights = fitter->Weights();
  meta->channels.resize(frequencies.size());
  for (size_t i = 0; i != frequencies.size(); ++i) {
    meta->channels[i].frequency = frequencies[i];
    meta->channels[i].weight = i < weights.size() ? weights[i] : 0.0;
  }
  meta->iteration_number = algorithm.IterationNumber();
  meta->final_threshold = algorithm.Threshold();
  meta->gain = algorithm.MinorLoopGain();
  meta->max_iterations = algorithm.MaxIterations();
  meta->major_iter_threshold = algorithm.MajorIterationThreshold();
  meta->mgain = algorithm.MajorLoopGain();
  meta->square_joined_channels = data_image.SquareJoinedChannels();
  return meta;
}

std::unique_ptr<algorithms::DeconvolutionAlgorithm> Factory(const std::string& filename) {
  return std::make_unique<algorithms::PythonDeconvolution>(filename);
}

bool InterpreterIsFinalizing() {
#if PY_VERSION_HEX >= 0x030D0000
  return Py_IsFinalizing() != 0;
#else
  return _Py_IsFinalizing() != 0;
#endif
}

// The keep-alive of imported planes: gives the tensor back to its producer.
// The teardown rules of ~PythonDeconvolution: a producer's deleter may touch
// Python objects, so it runs with the GIL or, once no thread can get the GIL
// any more, not at all (the memory goes with the process).
void ReleaseImported(void* pointer) {
  auto* tensor = static_cast<DLManagedTensor*>(pointer);
  if (!tensor || !tensor->deleter) return;
  if (!Py_IsInitialized()) return;
  if (PyGILState_Check()) {
    tensor->deleter(tensor);
    return;
  }
  if (InterpreterIsFinalizing()) return;
  py::gil_scoped_acquire gil;
  tensor->deleter(tensor);
}

std::shared_ptr<gpu::Session> ArraySession(const DeviceArray& a) {
  return gpu::Session::ForDevice(a.device);
}

}  // namespace

bool IsDlpackObject(const py::handle& object) {
  return !py::isinstance<py::array>(object) && py::hasattr(object, "__dlpack__");
}

DeviceImages ImportDeviceImages(const py::object& object, const std::string& argument) {
  const std::string name = "'" + argument + "'";
  const std::string rocm = "a ROCm device (DLPack device type " + std::to_string(int(kDLROCM)) + ")";
  if (!IsDlpackObject(object))
    throw py::type_error(name + " is a " + TypeName(object) +
                         ": a float32 numpy array or an object with __dlpack__ on " + rocm +
                         " is required");
  if (py::hasattr(object, "__dlpack_device__")) {
    // asked first: a host tensor is refused without being exported
    const py::tuple device = object.attr("__dlpack_device__")();
    if (device.size() != 2 || device[0].cast<int>() != int(kDLROCM))
      throw py::type_error(name + " is on DLPack device " + std::string(py::str(device)) +
                           ", not on " + rocm);
  }
  py::object capsule = object.attr("__dlpack__")();
  if (!PyCapsule_IsValid(capsule.ptr(), "dltensor"))
    throw py::type_error(name + ": its __dlpack__() did not return a 'dltensor' capsule");
  auto* managed =
      static_cast<DLManagedTensor*>(PyCapsule_GetPointer(capsule.ptr(), "dltensor"));
  const DLTensor& t = managed->dl_tensor;
  // (a refused capsule is still its producer's: its destructor releases it)
  if (t.device.device_type != kDLROCM)
    throw py::type_error(name + " is on DLPack device (" +
                         std::to_string(int(t.device.device_type)) + ", " +
                         std::to_string(t.device.device_id) + "), not on " + rocm);
  if (t.dtype.code != kDLFloat || t.dtype.bits != 32 || t.dtype.lanes != 1)
    throw py::type_error(name + " has dtype (code " + std::to_string(int(t.dtype.code)) + ", " +
                         std::to_string(int(t.dtype.bits)) + " bits), float32 is required");
  const size_t ndim = size_t(std::max(t.ndim, 0));
  const std::vector<int64_t> shape(t.shape, t.shape + ndim);
  if (t.strides) {
    const std::vector<int64_t> compact = CompactStrides(shape);
    for (size_t i = 0; i != ndim; ++i)
      if (shape[i] > 1 && t.strides[i] != compact[i])
        throw py::type_error(name + " is not C-contiguous (shape " + ShapeText(shape) +
                             ", strides " + ShapeText(t.strides, ndim) + " elements)");
  }
  if (!t.data && Count(shape) != 0) throw py::type_error(name + " has no data");
  // consumed from here on: the tensor is the keep-alive's to delete
  PyCapsule_SetName(capsule.ptr(), "used_dltensor");
  DeviceImages images;
  images.keep_alive = std::shared_ptr<void>(static_cast<void*>(managed), &ReleaseImported);
  images.data = reinterpret_cast<float*>(static_cast<char*>(t.data) + t.byte_offset);
  images.shape = shape;
  images.device = t.device.device_id;
  return images;
}

void InitPythonDeconvolution(py::module_& m) {
  py::module_ gpu = m.attr("gpu").cast<py::module_>();
  py::class_<DeviceArray>(
      gpu, "DeviceArray",
      "A float32, C-contiguous array in device memory: radler.gpu.to_device(array), or a view "
      "of an image set's own memory as passed to "
      "deconvolve_device(residual, model, psf, meta). Use it through DLPack "
      "(torch.from_dlpack(array)): the tensor shares the memory, so residual and model are "
      "edited in place; psf is read-only by contract. The view and every tensor made from "
      "it keep the allocation alive, but its contents are only meaningful during the call.")
      .def_property_readonly("shape",
                             [](const DeviceArray& a) {
                               py::tuple shape(a.shape.size());
                               for (size_t i = 0; i != a.shape.size(); ++i)
                                 shape[i] = py::int_(a.shape[i]);
                               return shape;
                             })
      .def_property_readonly("dtype", [](const DeviceArray&) { return "float32"; })
      .def_property_readonly(
          "data_ptr", [](const DeviceArray& a) { return reinterpret_cast<uintptr_t>(a.data); },
          "The device address of the first element.")
      .def(
          "numpy",
          [](const DeviceArray& a) {
            py::array_t<float> host(std::vector<py::ssize_t>(a.shape.begin(), a.shape.end()));
            float* h_dst = host.mutable_data();
            const size_t bytes = Count(a.shape) * sizeof(float);
            {
              py::gil_scoped_release release;
              const std::shared_ptr<gpu::Session> session = ArraySession(a);
              session->DeviceSync();  // whoever wrote it, on whatever stream
              if (bytes != 0) session->D2H(h_dst, a.data, bytes);
              session->Sync();
            }
            return host;
          },
          "A copy on the host (float32 numpy array), taken after the device has finished "
          "every queued operation.")
      .def(
          "view",
          [](const DeviceArray& a, size_t offset, const std::vector<int64_t>& shape) {
            for (int64_t d : shape)
              if (d < 0) throw std::runtime_error("DeviceArray.view: negative dimension");
            if (offset > Count(a.shape) || Count(shape) > Count(a.shape) - offset)
              throw std::runtime_error("DeviceArray.view: " + std::to_string(offset) + " + " +
                                       ShapeText(shape) + " elements do not fit in " +
                                       ShapeText(a.shape));
            return DeviceArray{a.buffer, a.data + offset, shape, a.device};
          },
          py::arg("offset"), py::arg("shape"),
          "A C-contiguous view of `shape` that starts `offset` elements into this array "
          "(4-byte granularity: the result need not be 16-byte aligned).")
      .def("__dlpack_device__",
           [](const DeviceArray& a) { return py::make_tuple(int(kDLROCM), a.device); })
      .def(
          "__dlpack__",
          [](const DeviceArray& a, const py::object& stream) {
            // The session was synchronised before the user's function was
            // called: the data is complete for any consumer stream.
            (void)stream;
            return ExportDlpack(a);
          },
          py::kw_only(), py::arg("stream") = py::none());

  gpu.def(
      "to_device",
      [](const py::array_t<float, py::array::c_style>& array, int device) {
        const std::shared_ptr<gpu::Session> session =
            gpu::Session::ForDevice(device >= 0 ? device : gpu::Session::DefaultDevice());
        DeviceArray out;
        out.shape.assign(array.shape(), array.shape() + array.ndim());
        out.device = session->Device();
        const size_t bytes = size_t(array.size()) * sizeof(float);
        const float* h_src = array.data();
        {
          py::gil_scoped_release release;
          out.buffer = std::make_shared<gpu::Buffer>(*session, std::max<size_t>(bytes, 16));
          if (bytes != 0) session->H2D(out.buffer->Ptr(), h_src, bytes);
          session->Sync();
        }
        out.data = out.buffer->F();
        return out;
      },
      py::arg("array").noconvert(), py::arg("device") = -1,
      "A float32 numpy array copied to the device (the process's session of `device`; -1: the "
      "default device) as a radler.gpu.DeviceArray, which radler.Radler and the WorkTableEntry "
      "setters accept in place of a numpy array.");

  py::module_ helpers = m.def_submodule(
      "python_deconvolution",
      "What a Python deconvolution function (Settings.Python.filename) is given as `meta`");
  py::class_<PyChannel>(helpers, "Channel")
      .def_readwrite("frequency", &PyChannel::frequency)
      .def_readwrite("weight", &PyChannel::weight);
  py::class_<PySpectralFitter>(helpers, "SpectralFitter")
      .def("fit", &PySpectralFitter::Fit, py::arg("values"), py::arg("x") = 0,
           py::arg("y") = 0)
      .def("fit_and_evaluate", &PySpectralFitter::FitAndEvaluate, py::arg("values"),
           py::arg("x") = 0, py::arg("y") = 0);
  py::class_<PyMetaData, std::shared_ptr<PyMetaData>>(helpers, "MetaData")
      .def_readonly("channels", &PyMetaData::channels)
      .def_readwrite("iteration_number", &PyMetaData::iteration_number)
      .def_readonly("final_threshold", &PyMetaData::final_threshold)
      .def_readonly("gain", &PyMetaData::gain)
      .def_readonly("max_iterations", &PyMetaData::max_iterations)
      .def_readonly("major_iter_threshold", &PyMetaData::major_iter_threshold)
      .def_readonly("mgain", &PyMetaData::mgain)
      .def_readonly("spectral_fitter", &PyMetaData::spectral_fitter)
      .def_readonly("square_joined_channels", &PyMetaData::square_joined_channels);

  algorithms::SetPythonDeconvolutionFactory(&Factory);
}

}  // namespace radler::python

namespace radler::algorithms {

using namespace radler::python;

PythonDeconvolution::PythonDeconvolution(const std::string& filename)
    : filename_(filename) {
  std::ifstream file(filename, std::ios::binary);
  if (!file)
    throw std::runtime_error("Python deconvolution: cannot open the file '" + filename + "'");
  const std::string source((std::istreambuf_iterator<char>(file)),
                           std::istreambuf_iterator<char>());
  py::gil_scoped_acquire gil;
  try {
    // a namespace of the file's own: the host's __main__ is someone else's
    py::dict scope;
    scope["__name__"] = "__radler_python_deconvolution__";
    scope["__file__"] = filename;
    scope["__builtins__"] = py::module_::import("builtins");
    py::object code = py::reinterpret_steal<py::object>(
        Py_CompileString(source.c_str(), filename.c_str(), Py_file_input));
    if (!code) throw py::error_already_set();
    py::object evaluated = py::reinterpret_steal<py::object>(
        PyEval_EvalCode(code.ptr(), scope.ptr(), scope.ptr()));
    if (!evaluated) throw py::error_already_set();
    py::object function;
    if (scope.contains("deconvolve_device")) {
      function = scope["deconvolve_device"];
      device_mode_ = true;
    } else if (scope.contains("deconvolve")) {
      function = scope["deconvolve"];
    } else {
      throw std::runtime_error(
          "Python deconvolution: '" + filename +
          "' defines neither deconvolve_device(residual, model, psf, meta) nor "
          "deconvolve(residual, model, psf, meta)");
    }
    if (!PyCallable_Check(function.ptr()))
      throw std::runtime_error("Python deconvolution: " +
                               std::string(device_mode_ ? "deconvolve_device" : "deconvolve") +
                               " in '" + filename + "' is not callable");
    function_ = function.release().ptr();
  } catch (py::error_already_set& e) {
    throw std::runtime_error("Python deconvolution: error while loading '" + filename +
                             "': " + e.what());
  }
}

PythonDeconvolution::PythonDeconvolution(const PythonDeconvolution& other)
    : DeconvolutionAlgorithm(other),
      filename_(other.filename_),
      device_mode_(other.device_mode_) {
  py::gil_scoped_acquire gil;
  function_ = other.function_;
  Py_XINCREF(function_);
}

PythonDeconvolution::~PythonDeconvolution() {
  if (!function_) return;
  // After the interpreter is gone the reference is leaked. While it
  // finalises, only the thread that holds the GIL (the module's teardown
  // destroying a Radler) can still give it back; no other thread will get
  // the GIL again.
  if (!Py_IsInitialized()) return;
  if (PyGILState_Check()) {
    Py_DECREF(function_);
    return;
  }
  if (InterpreterIsFinalizing()) return;
  py::gil_scoped_acquire gil;
  Py_DECREF(function_);
}

std::unique_ptr<DeconvolutionAlgorithm> PythonDeconvolution::Clone() const {
  return std::unique_ptr<DeconvolutionAlgorithm>(new PythonDeconvolution(*this));
}

DeconvolutionResult PythonDeconvolution::ExecuteMajorIteration(
    ImageSet& data_image, ImageSet& model_image, const gpu::Planes& psf_images) {
  // the sets of a grid's subimage live on its worker's session
  gpu::Session& s = data_image.Session();
  const size_t n_freq = data_image.NDeconvolutionChannels();
  const CallShape shape{n_freq, data_image.Size() / n_freq, data_image.Height(),
                        data_image.Width()};
  if (model_image.Size() != data_image.Size() || model_image.Width() != shape.width ||
      model_image.Height() != shape.height || &model_image.Session() != &s)
    throw std::runtime_error("Python deconvolution: residual and model image sets differ");
  if (psf_images.count != n_freq || psf_images.width != shape.width ||
      psf_images.height != shape.height || !psf_images.buffer)
    throw std::runtime_error(
        "Python deconvolution: one PSF of the image size per channel is required");
  // Everything queued on the session is done: the data may be read from any
  // stream (the device views), or converted and copied out (the host arrays).
  s.Sync();

  const char* const function_name = device_mode_ ? "deconvolve_device()" : "deconvolve()";
  py::gil_scoped_acquire gil;
  try {
    const std::shared_ptr<PyMetaData> meta = MakeMeta(*this, data_image);
    py::object residual, model, psf;
    if (device_mode_) {
      residual = py::cast(DeviceArray{data_image.Planes().buffer, data_image.Base(),
                                      shape.Images(), s.Device()});
      model = py::cast(DeviceArray{model_image.Planes().buffer, model_image.Base(),
                                   shape.Images(), s.Device()});
      psf = py::cast(
          DeviceArray{psf_images.buffer, psf_images.Base(), shape.Psfs(), s.Device()});
    } else {
      residual = ToHost(s, data_image.Base(), shape.Images());
      model = ToHost(s, model_image.Base(), shape.Images());
      psf = ToHost(s, psf_images.Base(), shape.Psfs());
    }

    py::object result;
    std::string call_error;
    bool call_failed = false;
    try {
      result = py::reinterpret_borrow<py::object>(function_)(residual, model, psf, meta);
    } catch (py::error_already_set& e) {
      call_failed = true;
      call_error = e.what();
    }
    {
      // The function may have launched on streams of its own (torch's), and
      // may have made another device current for this thread. Whether it
      // returned or raised, nothing of it may still run when the engine, or
      // the allocator that takes these planes back, goes on.
      py::gil_scoped_release release;
      s.DeviceSync();
    }
    if (call_failed) throw std::runtime_error(kCallErrorPrefix + call_error);
    SetIterationNumber(meta->iteration_number);

    if (!py::isinstance<py::dict>(result))
      BadResult("the return value of " + std::string(function_name) +
                " should be a dictionary, it is a " + TypeName(result));
    const py::dict dict = py::reinterpret_borrow<py::dict>(result);
    const std::vector<const char*> required =
        device_mode_ ? std::vector<const char*>{"level", "continue"}
                     : std::vector<const char*>{"residual", "model", "level", "continue"};
    for (const char* key : required)
      if (!dict.contains(key))
        BadResult("the dictionary returned by " + std::string(function_name) +
                  " has no '" + key + "' item; it should have " +
                  (device_mode_ ? "'level' and 'continue' (and may have 'residual' and 'model')"
                                : "'residual', 'model', 'level' and 'continue'"));
    DeconvolutionResult out;
    const py::object level_object = dict["level"], continue_object = dict["continue"];
    const double level = PyFloat_AsDouble(level_object.ptr());
    if (level == -1.0 && PyErr_Occurred()) {
      PyErr_Clear();
      BadResult("'level' returned by " + std::string(function_name) + " is a " +
                TypeName(level_object) + ", not a number");
    }
    out.final_peak_value = float(level);
    const int another = PyObject_IsTrue(continue_object.ptr());
    if (another < 0) {
      PyErr_Clear();
      BadResult("'continue' returned by " + std::string(function_name) + " has no truth value");
    }
    out.another_iteration_required = another != 0;

    if (device_mode_) {
      // the views were edited in place; only another array is copied
      struct Returned {
        const char* key;
        ImageSet* set;
        const py::object* passed;
      };
      for (const Returned& r : {Returned{"residual", &data_image, &residual},
                                Returned{"model", &model_image, &model}}) {
        if (!dict.contains(r.key)) continue;
        const py::object value = dict[r.key];
        if (value.is_none() || value.is(*r.passed)) continue;
        CopyFromDlpack(s, r.set->Base(), value, r.key, shape.Images());
      }
    } else {
      // both are checked before either set is written
      const py::object residual_object = dict["residual"], model_object = dict["model"];
      const py::array_t<double> new_residual =
          HostResult(residual_object, "residual", shape.Images());
      const py::array_t<double> new_model = HostResult(model_object, "model", shape.Images());
      FromHost(s, data_image.Base(), new_residual);
      FromHost(s, model_image.Base(), new_model);
    }
    return out;
  } catch (py::error_already_set& e) {
    throw std::runtime_error(kResultErrorPrefix + std::string(e.what()));
  }
}

}  // namespace radler::algorithms
