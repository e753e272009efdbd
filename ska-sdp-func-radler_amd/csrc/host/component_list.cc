#include "component_list.h"

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <limits>
#include <memory>
#include <numeric>
#include <stdexcept>

#ifdef RADLER_AMD_USE_EXTERNAL_AOCOMMON
#include <aocommon/imagecoordinates.h>
#include <aocommon/radeccoord.h>
#endif

#include "device.h"
#include "image_set.h"
#include "multiscale_algorithm.h"
#include "radler.h"
#include "spectral_fitter.h"

namespace radler {

ComponentList::ComponentList(size_t width, size_t height,
                             const ImageSet& model_set)
    : width_(width),
      height_(height),
      n_frequencies_(model_set.Size()),
      list_per_scale_(1) {
  const size_t n = width * height;
  std::vector<float> host(n * model_set.Size());
  model_set.Session().D2H(host.data(), model_set.Base(),
                          host.size() * sizeof(float));
  std::vector<float> values(n_frequencies_);
  for (size_t p = 0; p != n; ++p) {
    bool nonzero = false;
    for (size_t i = 0; i != n_frequencies_; ++i) {
      values[i] = host[i * n + p];
      nonzero = nonzero || values[i] != 0.0f;
    }
    if (nonzero) Add(p % width, p / width, 0, values.data());
  }
}

void ComponentList::Add(size_t x, size_t y, size_t scale_index,
                        const float* values) {
  ScaleList& l = list_per_scale_[scale_index];
  l.positions.push_back({x, y});
  l.values.insert(l.values.end(), values, values + n_frequencies_);
  if (++added_since_merge_ >= 100000) MergeDuplicates();
}

void ComponentList::Add(const ComponentList& other, int offset_x,
                        int offset_y) {
  if (other.NScales() > NScales()) SetNScales(other.NScales());
  for (size_t s = 0; s != other.NScales(); ++s) {
    const ScaleList& l = other.list_per_scale_[s];
    for (size_t i = 0; i != l.positions.size(); ++i)
      Add(l.positions[i].x + offset_x, l.positions[i].y + offset_y, s,
          &l.values[i * n_frequencies_]);
  }
}

void ComponentList::MergeDuplicates() {
  if (added_since_merge_ == 0) return;
  for (size_t s = 0; s != list_per_scale_.size(); ++s) MergeDuplicates(s);
  added_since_merge_ = 0;
}

void ComponentList::MergeDuplicates(size_t scale_index) {
  // component_list.h:222-263: the reference accumulates the values into one
  // image per frequency (in list order), then emits, frequency by frequency,
  // every raster position whose value in that frequency is non-zero (with
  // all its frequencies, which are then cleared). Positions whose summed
  // values are zero in every frequency disappear. Here a stable raster sort
  // sums duplicates in the same order; the emission passes follow.
  ScaleList& l = list_per_scale_[scale_index];
  std::vector<size_t> order(l.positions.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    const Position& pa = l.positions[a];
    const Position& pb = l.positions[b];
    return pa.y != pb.y ? pa.y < pb.y : pa.x < pb.x;
  });
  ScaleList merged;
  for (size_t idx : order) {
    const Position& p = l.positions[idx];
    if (!merged.positions.empty() && merged.positions.back().x == p.x &&
        merged.positions.back().y == p.y) {
      float* dst = &merged.values[merged.values.size() - n_frequencies_];
      for (size_t f = 0; f != n_frequencies_; ++f)
        dst[f] += l.values[idx * n_frequencies_ + f];
    } else {
      merged.positions.push_back(p);
      merged.values.insert(merged.values.end(),
                           l.values.begin() + idx * n_frequencies_,
                           l.values.begin() + (idx + 1) * n_frequencies_);
    }
  }
  ScaleList out;
  std::vector<char> emitted(merged.positions.size(), 0);
  for (size_t f = 0; f != n_frequencies_; ++f)
    for (size_t i = 0; i != merged.positions.size(); ++i) {
      if (emitted[i] || merged.values[i * n_frequencies_ + f] == 0.0f) continue;
      emitted[i] = 1;
      out.positions.push_back(merged.positions[i]);
      out.values.insert(out.values.end(), merged.values.begin() + i * n_frequencies_,
                        merged.values.begin() + (i + 1) * n_frequencies_);
    }
  l = std::move(out);
}

void ComponentList::MultiplyScaleComponent(size_t scale_index, size_t position_index,
                                           size_t channel, double correction_factor) {
  float& value =
      list_per_scale_[scale_index].values[channel + position_index * n_frequencies_];
  value *= correction_factor;  // component_list.h:178-186 (float *= double)
}

void ComponentList::SetValues(size_t scale_index, size_t index, const float* values) {
  std::copy_n(values, n_frequencies_,
              &list_per_scale_[scale_index].values[index * n_frequencies_]);
}

// ------------------------------------------------------- source catalogue
namespace {

using schaapcommon::fitters::SpectralFitter;
using schaapcommon::fitters::SpectralFittingMode;

constexpr int kFloatDigits = std::numeric_limits<float>::digits10 + 1;    // 7
constexpr int kDoubleDigits = std::numeric_limits<double>::digits10 + 1;  // 16

// cpp/utils/write_model.h: the text format of a source catalogue
void WriteHeader(std::ostream& stream, double reference_frequency) {
  stream.precision(kDoubleDigits);
  stream << "Format = Name, Type, Ra, Dec, I, SpectralIndex, LogarithmicSI, "
            "ReferenceFrequency='"
         << reference_frequency << "', MajorAxis, MinorAxis, Orientation\n";
}

// name,TYPE,ra,dec,t0,[t1,...],true|false,ref, then the shape: empty fields
// for a point, major and minor axis (arcsec) and orientation for a Gaussian
void WriteRow(std::ostream& stream, size_t scale_index, size_t component_index,
              bool gaussian, long double ra, long double dec, const float* terms,
              size_t n_terms, bool use_log_si, double reference_frequency, double major,
              double minor) {
  stream << 's' << scale_index << 'c' << component_index
         << (gaussian ? ",GAUSSIAN," : ",POINT,") << aocommon::RaDecCoord::RAToString(ra, ':')
         << ',' << aocommon::RaDecCoord::DecToString(dec, '.') << ',';
  stream << std::setprecision(kFloatDigits) << terms[0] << ",[";
  for (size_t t = 1; t < n_terms; ++t) {
    if (t != 1) stream << ',';
    stream << terms[t];
  }
  stream << ']';
  stream.precision(kDoubleDigits);
  stream << ',' << (use_log_si ? "true" : "false") << ',' << reference_frequency << ',';
  if (gaussian)
    stream << major << ',' << minor << ',' << 0.0 << '\n';
  else
    stream << ",,\n";
}

}  // namespace

size_t ComponentList::TermCount(const SpectralFitter& fitter) const {
  return n_frequencies_ == 1 ? 1 : fitter.NTerms();
}

void ComponentList::CheckWritable(const SpectralFitter& fitter) const {
  if (added_since_merge_ != 0)
    throw std::runtime_error(
        "ComponentList::Write called while there are yet unmerged components. "
        "Run ComponentList::MergeDuplicates() first.");
  if (fitter.Mode() == SpectralFittingMode::kNoFitting && n_frequencies_ > 1)
    throw std::runtime_error(
        "Can't Write component list, because you have not specified a spectral "
        "fitting method. You probably want to add '-fit-spectral-pol'.");
  if (n_frequencies_ > 1 && fitter.Frequencies().size() != n_frequencies_)
    throw std::runtime_error(
        "Can't Write component list: its components have " +
        std::to_string(n_frequencies_) + " frequencies, the spectral fitter has " +
        std::to_string(fitter.Frequencies().size()) + " channels");
  if (n_frequencies_ > 1 && fitter.NTerms() == 0)
    throw std::runtime_error("Can't Write component list: the spectral fitter has no terms");
}

// What the device fit of one Write needs, made once and used for every
// scale: the fitter's description and, for a forced fit, the term planes on
// the device (one upload, however many scales the list has).
struct ComponentList::DeviceFit {
  gpu::Session& session;
  uint32_t mode = RDL_TERMS_POLYNOMIAL;
  std::vector<double> map;      // polynomial: n_terms x n_channels
  std::vector<uint8_t> fitted;  // polynomial: channel has weight > 0
  rdl_logpoly fit{};            // log-polynomial, forced
  rdl_forced_terms forced{};    // forced
  gpu::Buffer planes;           // forced: what forced.d_planes points at
};

std::unique_ptr<ComponentList::DeviceFit> ComponentList::MakeDeviceFit(
    const SpectralFitter& fitter, gpu::Session& session, const ForcedTermImages* images) const {
  auto fit = std::make_unique<DeviceFit>(DeviceFit{session});
  session.Bind();
  switch (fitter.Mode()) {
    case SpectralFittingMode::kNoFitting:
      break;  // CheckWritable: a single frequency, nothing is fitted
    case SpectralFittingMode::kPolynomial:
      fit->mode = RDL_TERMS_POLYNOMIAL;
      fit->map = MakeSpectralMaps(fitter).fit;
      fit->fitted.resize(n_frequencies_);
      for (size_t c = 0; c != n_frequencies_; ++c)
        fit->fitted[c] = c < fitter.Weights().size() && fitter.Weights()[c] > 0.0f;
      break;
    case SpectralFittingMode::kLogPolynomial:
      fit->mode = RDL_TERMS_LOGPOLY;
      MakeLogPoly(fitter, &fit->fit);
      break;
    case SpectralFittingMode::kForcedTerms: {
      fit->mode = RDL_TERMS_FORCED;
      MakeForcedLogPoly(fitter, &fit->fit, fit->forced.weights);
      if (fitter.NTerms() <= 1) break;
      // full-image planes: the algorithm's (contiguous), or the fitter's own
      std::vector<const float*> planes;
      size_t width = 0, plane = 0;
      if (images) {
        width = images->width;
        plane = images->width * images->height;
        for (size_t k = 0; k != images->n_planes; ++k)
          planes.push_back(images->data.data() + k * plane);
      }
#ifndef RADLER_AMD_USE_EXTERNAL_AOCOMMON
      else {
        width = fitter.ForcedWidth();
        for (const std::vector<float>& p : fitter.ForcedPlanes()) {
          planes.push_back(p.data());
          plane = p.size();
        }
      }
#endif
      if (planes.size() + 1 != fitter.NTerms() || width == 0)
        throw std::runtime_error(
            "ComponentList::Write: forced-term fitting needs the term planes of the image");
      fit->planes = gpu::Buffer(session, planes.size() * plane * sizeof(float));
      for (size_t k = 0; k != planes.size(); ++k)
        session.H2D(fit->planes.F() + k * plane, planes[k], plane * sizeof(float));
      fit->forced.d_planes = fit->planes.F();
      fit->forced.plane_stride = plane;
      fit->forced.pitch = uint32_t(width);
      fit->forced.rows = uint32_t(plane / width);
      break;
    }
  }
  return fit;
}

void ComponentList::FitTermsIntoDevice(size_t scale_index, size_t n_terms, const DeviceFit& fit,
                                       gpu::Buffer& d_terms) const {
  const ScaleList& list = list_per_scale_[scale_index];
  const size_t n = list.positions.size();
  if (n == 0) return;
  // channel-major spectra in, term-major terms out
  gpu::Session& s = fit.session;
  s.Bind();
  std::vector<float> staged(n * n_frequencies_);
  for (size_t i = 0; i != n; ++i)
    for (size_t f = 0; f != n_frequencies_; ++f)
      staged[f * n + i] = list.values[i * n_frequencies_ + f];
  gpu::Buffer d_values(s, n * n_frequencies_ * sizeof(float));
  d_terms.Resize(s, n * n_terms * sizeof(float));
  s.H2D(d_values.Ptr(), staged.data(), n * n_frequencies_ * sizeof(float));
  std::vector<uint32_t> xy;
  if (fit.mode == RDL_TERMS_FORCED) {
    xy.resize(2 * n);
    for (size_t i = 0; i != n; ++i) {
      xy[i] = uint32_t(list.positions[i].x);
      xy[n + i] = uint32_t(list.positions[i].y);
    }
  }
  gpu::Check(rdl_component_terms(s.Handle(), fit.mode, uint32_t(n_frequencies_),
                                 uint32_t(n_terms), fit.map.data(), fit.fitted.data(), &fit.fit,
                                 &fit.forced, uint32_t(width_), uint32_t(height_), xy.data(),
                                 xy.empty() ? nullptr : xy.data() + n, d_values.F(), n, n,
                                 d_terms.F(), n),
             "rdl_component_terms");
  // d_values is released in stream order, after the fit that reads it
}

std::vector<float> ComponentList::FitTermsOnDevice(size_t scale_index, size_t n_terms,
                                                   const DeviceFit& fit) const {
  const size_t n = list_per_scale_[scale_index].positions.size();
  std::vector<float> terms(n * n_terms);
  if (n == 0) return terms;
  gpu::Buffer d_terms;
  FitTermsIntoDevice(scale_index, n_terms, fit, d_terms);
  std::vector<float> staged(n * n_terms);
  fit.session.D2H(staged.data(), d_terms.Ptr(), n * n_terms * sizeof(float));
  for (size_t i = 0; i != n; ++i)
    for (size_t t = 0; t != n_terms; ++t) terms[i * n_terms + t] = staged[t * n + i];
  return terms;
}

std::vector<float> ComponentList::FitTermsOnHost(size_t scale_index, size_t n_terms,
                                                 const SpectralFitter& fitter) const {
  const ScaleList& list = list_per_scale_[scale_index];
  const size_t n = list.positions.size();
  std::vector<float> terms(n * n_terms), one;
  for (size_t i = 0; i != n; ++i) {
    fitter.Fit(one, &list.values[i * n_frequencies_], list.positions[i].x, list.positions[i].y);
    std::copy_n(one.begin(), n_terms, &terms[i * n_terms]);
  }
  return terms;
}

std::vector<float> ComponentList::FitTerms(size_t scale_index, const SpectralFitter& fitter,
                                           gpu::Session* session) const {
  CheckWritable(fitter);
  if (n_frequencies_ == 1) return list_per_scale_[scale_index].values;
  if (!session) return FitTermsOnHost(scale_index, TermCount(fitter), fitter);
  return FitTermsOnDevice(scale_index, TermCount(fitter),
                          *MakeDeviceFit(fitter, *session, nullptr));
}

void ComponentList::WriteSources(const Radler& radler, const std::string& filename,
                                 long double pixel_scale_x, long double pixel_scale_y,
                                 long double phase_centre_ra, long double phase_centre_dec,
                                 long double l_shift, long double m_shift) const {
  const algorithms::DeconvolutionAlgorithm& algorithm = radler.MaxScaleCountAlgorithm();
  std::vector<double> scale_sizes(NScales(), 0.0);
  if (const auto* multiscale = dynamic_cast<const algorithms::MultiScaleAlgorithm*>(&algorithm))
    for (size_t i = 0; i != NScales(); ++i) scale_sizes[i] = multiscale->ScaleSize(i);
  else
    scale_sizes.assign(1, 0.0);
  const SpectralFitter& fitter = algorithm.Fitter();
  // nothing is fitted for a single frequency
  gpu::Session* session = n_frequencies_ > 1 ? &radler.DeviceSession() : nullptr;
  // the algorithm, not its fitter, holds the full-image term planes of a forced fit
  WriteRows(filename, fitter, scale_sizes, pixel_scale_x, pixel_scale_y, phase_centre_ra,
            phase_centre_dec, l_shift, m_shift, session, algorithm.SpectrallyForcedImages().get());
}

void ComponentList::Write(const std::string& filename,
                          const algorithms::MultiScaleAlgorithm& multiscale,
                          long double pixel_scale_x, long double pixel_scale_y,
                          long double phase_centre_ra, long double phase_centre_dec,
                          long double l_shift, long double m_shift) const {
  std::vector<double> scale_sizes(NScales());
  for (size_t i = 0; i != NScales(); ++i) scale_sizes[i] = multiscale.ScaleSize(i);
  Write(filename, multiscale.Fitter(), scale_sizes, pixel_scale_x, pixel_scale_y,
        phase_centre_ra, phase_centre_dec, l_shift, m_shift);
}

void ComponentList::WriteSingleScale(const std::string& filename,
                                     const algorithms::DeconvolutionAlgorithm& algorithm,
                                     long double pixel_scale_x, long double pixel_scale_y,
                                     long double phase_centre_ra, long double phase_centre_dec,
                                     long double l_shift, long double m_shift) const {
  Write(filename, algorithm.Fitter(), std::vector<double>(1, 0.0), pixel_scale_x, pixel_scale_y,
        phase_centre_ra, phase_centre_dec, l_shift, m_shift);
}

void ComponentList::Write(const std::string& filename, const SpectralFitter& fitter,
                          const std::vector<double>& scale_sizes, long double pixel_scale_x,
                          long double pixel_scale_y, long double phase_centre_ra,
                          long double phase_centre_dec, long double l_shift,
                          long double m_shift, gpu::Session* session) const {
  WriteRows(filename, fitter, scale_sizes, pixel_scale_x, pixel_scale_y, phase_centre_ra,
            phase_centre_dec, l_shift, m_shift, session, nullptr);
}

void ComponentList::WriteRows(const std::string& filename, const SpectralFitter& fitter,
                              const std::vector<double>& scale_sizes,
                              long double pixel_scale_x, long double pixel_scale_y,
                              long double phase_centre_ra, long double phase_centre_dec,
                              long double l_shift, long double m_shift, gpu::Session* session,
                              const ForcedTermImages* images) const {
  CheckWritable(fitter);
  std::unique_ptr<DeviceFit> device_fit;
  if (session && n_frequencies_ > 1) device_fit = MakeDeviceFit(fitter, *session, images);
  if (scale_sizes.size() < NScales())
    throw std::runtime_error("ComponentList::Write: " + std::to_string(scale_sizes.size()) +
                             " scale sizes given for " + std::to_string(NScales()) +
                             " scales");
  const bool use_log_si = fitter.Mode() == SpectralFittingMode::kLogPolynomial ||
                          fitter.Mode() == SpectralFittingMode::kForcedTerms;
  const size_t n_terms = TermCount(fitter);
  const double reference = fitter.ReferenceFrequency();
  std::ofstream file(filename);
  if (!file) throw std::runtime_error("ComponentList::Write: can't open " + filename);
  WriteHeader(file, reference);
  for (size_t scale_index = 0; scale_index != NScales(); ++scale_index) {
    const ScaleList& list = list_per_scale_[scale_index];
    const double scale = scale_sizes[scale_index];
    // the FWHM of the scale's Gaussian, in arcsec along each axis
    const double fwhm =
        2.0L * std::sqrt(2.0L * std::log(2.0L)) *
        algorithms::multiscale::MultiScaleTransforms::GaussianSigma(scale);
    const double major = fwhm * pixel_scale_x * (180.0 * 60.0 * 60.0 / M_PI),
                 minor = fwhm * pixel_scale_y * (180.0 * 60.0 * 60.0 / M_PI);
    const std::vector<float> terms =
        n_frequencies_ == 1 ? list.values
        : device_fit        ? FitTermsOnDevice(scale_index, n_terms, *device_fit)
                            : FitTermsOnHost(scale_index, n_terms, fitter);
    for (size_t index = 0; index != list.positions.size(); ++index) {
      const size_t x = list.positions[index].x, y = list.positions[index].y;
      long double l, m, ra, dec;
      aocommon::ImageCoordinates::XYToLM<long double>(x, y, pixel_scale_x, pixel_scale_y,
                                                      width_, height_, l, m);
      l += l_shift;
      m += m_shift;
      aocommon::ImageCoordinates::LMToRaDec<long double>(l, m, phase_centre_ra,
                                                         phase_centre_dec, ra, dec);
      WriteRow(file, scale_index, index, scale != 0.0, ra, dec, &terms[index * n_terms],
               n_terms, use_log_si, reference, major, minor);
    }
  }
  if (!file) throw std::runtime_error("ComponentList::Write: writing " + filename + " failed");
}

// ------------------------------------------------------------ model images
void ComponentList::CheckRender(const SpectralFitter& fitter,
                                const std::vector<double>& scale_sizes,
                                const std::vector<double>& frequencies) const {
  if (added_since_merge_ != 0)
    throw std::runtime_error(
        "ComponentList::Render called while there are yet unmerged components. "
        "Run ComponentList::MergeDuplicates() first.");
  if (scale_sizes.size() != NScales())
    throw std::runtime_error("ComponentList::Render: " + std::to_string(scale_sizes.size()) +
                             " scale sizes given for " + std::to_string(NScales()) + " scales");
  for (double frequency : frequencies)
    if (!(frequency > 0.0))
      throw std::runtime_error("ComponentList::Render: a frequency is not positive");
  // the list's own values need no fitter; terms come from the fit Write uses
  const bool values = frequencies.empty();
  const bool fitted = !values && n_frequencies_ > 1;
  if (fitted) CheckWritable(fitter);
  // a fitter that fits at all must be the list's, used or not
  if (n_frequencies_ > 1 && fitter.Mode() != SpectralFittingMode::kNoFitting &&
      fitter.Frequencies().size() != n_frequencies_)
    throw std::runtime_error("ComponentList::Render: the components have " +
                             std::to_string(n_frequencies_) +
                             " frequencies, the spectral fitter has " +
                             std::to_string(fitter.Frequencies().size()) + " channels");
  const size_t n_out = values ? n_frequencies_ : frequencies.size();
  if (n_out > RDL_MAX_IMAGES)
    throw std::runtime_error("ComponentList::Render: more than " +
                             std::to_string(RDL_MAX_IMAGES) + " planes asked for");
}

std::vector<aocommon::Image> ComponentList::Render(const Radler& radler,
                                                   const std::vector<double>& frequencies) const {
  const algorithms::DeconvolutionAlgorithm& algorithm = radler.MaxScaleCountAlgorithm();
  std::vector<double> scale_sizes(NScales(), 0.0);
  if (const auto* multiscale = dynamic_cast<const algorithms::MultiScaleAlgorithm*>(&algorithm))
    for (size_t i = 0; i != NScales(); ++i) scale_sizes[i] = multiscale->ScaleSize(i);
  return Render(algorithm.Fitter(), scale_sizes, radler.GetSettings().multiscale.shape,
                frequencies, radler.DeviceSession(), algorithm.SpectrallyForcedImages().get());
}

std::vector<aocommon::Image> ComponentList::Render(const SpectralFitter& fitter,
                                                   const std::vector<double>& scale_sizes,
                                                   MultiscaleShape shape,
                                                   const std::vector<double>& frequencies,
                                                   gpu::Session& session) const {
  return Render(fitter, scale_sizes, shape, frequencies, session, nullptr);
}

std::vector<aocommon::Image> ComponentList::Render(const SpectralFitter& fitter,
                                                   const std::vector<double>& scale_sizes,
                                                   MultiscaleShape shape,
                                                   const std::vector<double>& frequencies,
                                                   gpu::Session& session,
                                                   const ForcedTermImages* images) const {
  using algorithms::multiscale::MultiScaleTransforms;
  CheckRender(fitter, scale_sizes, frequencies);
  // the list's own values need no fitter; terms come from the fit Write uses
  const bool values = frequencies.empty();
  const bool fitted = !values && n_frequencies_ > 1;
  const size_t n_out = values ? n_frequencies_ : frequencies.size();
  std::vector<aocommon::Image> result;
  if (n_out == 0 || width_ == 0 || height_ == 0) return result;

  // what rdl_render_components evaluates the rows at (SpectralFitter::Evaluate)
  uint32_t mode = RDL_RENDER_VALUES;
  std::vector<double> at;
  if (!values) {
    const bool log_si = fitted && (fitter.Mode() == SpectralFittingMode::kLogPolynomial ||
                                   fitter.Mode() == SpectralFittingMode::kForcedTerms);
    // a single-frequency list: one term, its value, whatever the frequency
    mode = log_si ? RDL_TERMS_LOGPOLY : RDL_TERMS_POLYNOMIAL;
    for (double frequency : frequencies) {
      const double ratio = fitted ? frequency / fitter.ReferenceFrequency() : 1.0;
      at.push_back(log_si ? std::log10(ratio) : ratio - 1.0);
    }
  }
  const size_t n_rows = values ? n_frequencies_ : TermCount(fitter);

  gpu::Session& s = session;
  s.Bind();
  const size_t plane = width_ * height_;
  MultiScaleTransforms transforms(s, width_, height_, shape);
  float max_scale = 0.0f;
  for (size_t scale = 0; scale != NScales(); ++scale)
    if (ComponentCount(scale) != 0) max_scale = std::max(max_scale, float(scale_sizes[scale]));
  if (max_scale != 0.0f) transforms.SetMaxScale(max_scale);
  std::unique_ptr<DeviceFit> device_fit;
  if (fitted) device_fit = MakeDeviceFit(fitter, s, images);

  gpu::Buffer out(s, n_out * plane * sizeof(float)), delta(s, n_out * plane * sizeof(float));
  gpu::Check(rdl_memset_zero(s.Handle(), out.Ptr(), n_out * plane * sizeof(float)),
             "rdl_memset_zero");
  // summed in the spectrum: one accumulator per plane, the transform of one
  // delta plane at a time
  gpu::Buffer accumulators, spectrum, rows;
  size_t spectrum_bytes = 0;
  bool accumulated = false;
  std::vector<uint32_t> xy;
  std::vector<float> staged;
  for (size_t scale = 0; scale != NScales(); ++scale) {
    const ScaleList& list = list_per_scale_[scale];
    const size_t n = list.positions.size();
    if (n == 0) continue;
    xy.resize(2 * n);
    for (size_t i = 0; i != n; ++i) {
      xy[i] = uint32_t(list.positions[i].x);
      xy[n + i] = uint32_t(list.positions[i].y);
    }
    if (fitted) {  // the terms stay on the device between the fit and the render
      FitTermsIntoDevice(scale, n_rows, *device_fit, rows);
    } else {
      staged.resize(n * n_frequencies_);
      for (size_t i = 0; i != n; ++i)
        for (size_t f = 0; f != n_frequencies_; ++f)
          staged[f * n + i] = list.values[i * n_frequencies_ + f];
      rows.Resize(s, staged.size() * sizeof(float));
      s.H2D(rows.Ptr(), staged.data(), staged.size() * sizeof(float));
    }
    gpu::Check(rdl_render_components(s.Handle(), mode, uint32_t(n_rows), rows.F(), n, n,
                                     xy.data(), xy.data() + n, uint32_t(width_),
                                     uint32_t(height_), values ? nullptr : at.data(),
                                     uint32_t(n_out), delta.F(), plane),
               "rdl_render_components");
    const float size = float(scale_sizes[scale]);
    if (size == 0.0f) {
      gpu::Check(rdl_add(s.Handle(), out.F(), delta.F(), n_out * plane), "rdl_add");
      continue;
    }
    const void* kernel = transforms.KernelSpectrum(size);
    if (spectrum_bytes == 0) {
      spectrum_bytes = transforms.SpectrumBytes();
      accumulators.Resize(s, n_out * spectrum_bytes);
      spectrum.Resize(s, spectrum_bytes);
    }
    // every element of the spectrum's storage, whatever its layout
    const size_t n_complex = spectrum_bytes / (2 * sizeof(float));
    for (size_t g = 0; g != n_out; ++g) {
      void* accumulator = static_cast<char*>(accumulators.Ptr()) + g * spectrum_bytes;
      transforms.Forward(delta.F() + g * plane, spectrum.Ptr());
      if (!accumulated)
        gpu::Check(rdl_spectrum_multiply(s.Handle(), accumulator, spectrum.Ptr(), kernel,
                                         n_complex, 1.0f),
                   "rdl_spectrum_multiply");
      else
        gpu::Check(rdl_spectrum_multiply_add(s.Handle(), accumulator, spectrum.Ptr(), kernel,
                                             n_complex, 1.0f),
                   "rdl_spectrum_multiply_add");
    }
    accumulated = true;
  }
  if (accumulated) {
    // the one inverse: ConvolveSpectrum with the size-0 kernel, whose
    // spectrum is 1 everywhere (a delta at the origin), so only the
    // normalisation and the inverse transform act on the sum
    for (size_t g = 0; g != n_out; ++g)
      transforms.ConvolveSpectrum(static_cast<char*>(accumulators.Ptr()) + g * spectrum_bytes,
                                  0.0f, spectrum.Ptr(), delta.F() + g * plane);
    gpu::Check(rdl_add(s.Handle(), out.F(), delta.F(), n_out * plane), "rdl_add");
  }
  // the copies back wait for the device anyway; queued behind the pending
  // kernels instead, the 8192^2 plane's copy took 17 ms, after this 5 ms
  // (profiles/render_restore_timing.txt)
  s.Sync();
  for (size_t g = 0; g != n_out; ++g) {
    result.emplace_back(width_, height_);
    s.D2H(result.back().Data(), out.F() + g * plane, plane * sizeof(float));
  }
  return result;
}

void ComponentList::Clear() {
  for (ScaleList& l : list_per_scale_) {
    l.positions.clear();
    l.values.clear();
  }
  added_since_merge_ = 0;
}

void ComponentList::GetComponent(size_t scale_index, size_t index, size_t& x,
                                 size_t& y, float* values) const {
  const ScaleList& l = list_per_scale_[scale_index];
  x = l.positions[index].x;
  y = l.positions[index].y;
  std::copy_n(&l.values[index * n_frequencies_], n_frequencies_, values);
}

}  // namespace radler
