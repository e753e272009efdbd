// radler::ComponentList (reference: cpp/component_list.{h,cc}): per-scale
// component positions with one value per image. Built from the model images
// for single-scale algorithms; recorded by MultiScaleAlgorithm otherwise.
#pragma once

#include <cstddef>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "aocommon_compat.h"
#include "settings.h"

#ifndef RADLER_AMD_USE_EXTERNAL_AOCOMMON
namespace schaapcommon::fitters {
class SpectralFitter;
}
#else
#include <schaapcommon/fitters/spectralfitter.h>
#endif

namespace radler {

class ImageSet;
class Radler;
struct ForcedTermImages;
namespace algorithms {
class DeconvolutionAlgorithm;
class MultiScaleAlgorithm;
}  // namespace algorithms
namespace gpu {
class Buffer;
class Session;
}

class ComponentList {
 public:
  ComponentList() = default;
  ComponentList(size_t width, size_t height, size_t n_scales,
                size_t n_frequencies)
      : width_(width),
        height_(height),
        n_frequencies_(n_frequencies),
        list_per_scale_(n_scales) {}
  /// Every non-zero model pixel becomes a scale-0 component
  /// (component_list.h:46-55 LoadFromImageSet).
  ComponentList(size_t width, size_t height, const ImageSet& model_set);

  struct Position {
    size_t x, y;
  };

  void Add(size_t x, size_t y, size_t scale_index, const float* values);
  void Add(const ComponentList& other, int offset_x, int offset_y);
  void MergeDuplicates();
  void Clear();
  size_t Width() const { return width_; }
  size_t Height() const { return height_; }
  size_t NScales() const { return list_per_scale_.size(); }
  void SetNScales(size_t n) { list_per_scale_.resize(n); }
  size_t NFrequencies() const { return n_frequencies_; }
  size_t ComponentCount(size_t scale_index) const {
    return list_per_scale_[scale_index].positions.size();
  }
  void GetComponent(size_t scale_index, size_t index, size_t& x, size_t& y,
                    float* values) const;
  std::pair<size_t, size_t> GetComponentPosition(size_t scale_index, size_t index) const {
    const auto& p = list_per_scale_[scale_index].positions[index];
    return {p.x, p.y};
  }
  /// GetSingleValue (component_list.h): value of image `image_index`
  float& Value(size_t scale_index, size_t index, size_t image_index) {
    return list_per_scale_[scale_index].values[index * n_frequencies_ + image_index];
  }
  /// component_list.h:157-164
  void SetValues(size_t scale_index, size_t index, const float* values);
  /// component_list.h:178-186 (primary-beam correction factors)
  void MultiplyScaleComponent(size_t scale_index, size_t position_index,
                              size_t channel, double correction_factor);
  /// component_list.h:191-194
  const std::vector<Position>& GetPositions(size_t scale_index) const {
    return list_per_scale_[scale_index].positions;
  }

  /// component_list.cc:15-32: the list as a source catalogue (text), with the
  /// scale sizes and the spectral fitter of the Radler's algorithm. The
  /// spectral terms are fitted on the Radler's device session: in every
  /// fitting mode the batched fit, with its staging, its copies and (forced)
  /// one upload of term planes of the image's size, is faster than the host
  /// loop at the list sizes of a deep clean (profiles/component_terms_fit.txt).
  void WriteSources(const Radler& radler, const std::string& filename,
                    long double pixel_scale_x, long double pixel_scale_y,
                    long double phase_centre_ra, long double phase_centre_dec,
                    long double l_shift = 0.0, long double m_shift = 0.0) const;
  /// component_list.cc:34-57
  void Write(const std::string& filename, const algorithms::MultiScaleAlgorithm& multiscale,
             long double pixel_scale_x, long double pixel_scale_y,
             long double phase_centre_ra, long double phase_centre_dec,
             long double l_shift = 0.0, long double m_shift = 0.0) const;
  void WriteSingleScale(const std::string& filename,
                        const algorithms::DeconvolutionAlgorithm& algorithm,
                        long double pixel_scale_x, long double pixel_scale_y,
                        long double phase_centre_ra, long double phase_centre_dec,
                        long double l_shift = 0.0, long double m_shift = 0.0) const;
  /// component_list.cc:59-140. One row per component: POINT for a scale of
  /// size 0, GAUSSIAN otherwise. Without a session every component is fitted
  /// by fitter.Fit on the host, as the reference does; with one, a scale's
  /// components are fitted in one batch on the device
  /// (rdl_component_terms). The rows are formatted by the same code, so the
  /// two files differ in nothing but the fitted terms. Unlike the reference
  /// this throws when the list has several frequencies and the fitter has
  /// another number of channels (the reference fits a spectrum of the wrong
  /// length).
  void Write(const std::string& filename,
             const schaapcommon::fitters::SpectralFitter& fitter,
             const std::vector<double>& scale_sizes, long double pixel_scale_x,
             long double pixel_scale_y, long double phase_centre_ra,
             long double phase_centre_dec, long double l_shift = 0.0,
             long double m_shift = 0.0, gpu::Session* session = nullptr) const;
  /// The terms Write gives the components of a scale, component by component
  /// (TermCount(fitter) floats each); the same two paths.
  std::vector<float> FitTerms(size_t scale_index,
                              const schaapcommon::fitters::SpectralFitter& fitter,
                              gpu::Session* session = nullptr) const;
  /// Terms per component: the fitter's, or 1 for a single-frequency list
  /// (its value is its only term and nothing is fitted).
  size_t TermCount(const schaapcommon::fitters::SpectralFitter& fitter) const;

  /// The list as model images on the device session: plane g = the sum over
  /// the scales of (the scale's delta plane convolved with its shape kernel),
  /// the convolution circular at Width() x Height() as MultiScaleAlgorithm
  /// applies it to its own model (MultiScaleTransforms); a scale of size 0 is
  /// added as it is. With `frequencies` empty the planes are the list's own
  /// values, one per list frequency. Otherwise plane g is the list at
  /// frequencies[g] (Hz): every component's terms, those Write prints
  /// (FitTerms on the device, in any fitting mode), evaluated as
  /// fitter.Evaluate does; a single-frequency list has its value as its only
  /// term and gives the same plane at every frequency. The products of the
  /// scales' spectra are summed and inverted once: a plane costs one forward
  /// transform per non-zero scale that holds components, and one inverse.
  /// Throws, before the first device call, on an unmerged list, a scale-size
  /// count other than NScales(), a fitter whose channels are not the list's
  /// and a frequency <= 0. The second form takes the fitter, the scale sizes,
  /// the shape, the forced-term planes and the session of the Radler.
  std::vector<aocommon::Image> Render(const schaapcommon::fitters::SpectralFitter& fitter,
                                      const std::vector<double>& scale_sizes,
                                      MultiscaleShape shape,
                                      const std::vector<double>& frequencies,
                                      gpu::Session& session) const;
  std::vector<aocommon::Image> Render(const Radler& radler,
                                      const std::vector<double>& frequencies = {}) const;
  /// Render's checks of its arguments, on their own: throws what Render
  /// would, and touches no device.
  void CheckRender(const schaapcommon::fitters::SpectralFitter& fitter,
                   const std::vector<double>& scale_sizes,
                   const std::vector<double>& frequencies) const;

 private:
  std::vector<aocommon::Image> Render(const schaapcommon::fitters::SpectralFitter& fitter,
                                      const std::vector<double>& scale_sizes,
                                      MultiscaleShape shape,
                                      const std::vector<double>& frequencies,
                                      gpu::Session& session,
                                      const ForcedTermImages* images) const;
  struct ScaleList {
    std::vector<Position> positions;
    std::vector<float> values;
  };
  void MergeDuplicates(size_t scale_index);
  void CheckWritable(const schaapcommon::fitters::SpectralFitter& fitter) const;
  struct DeviceFit;
  /// `images`: the full-image term planes of a forced fit on the device when
  /// the fitter does not hold them itself (a Radler's algorithm keeps them)
  std::unique_ptr<DeviceFit> MakeDeviceFit(const schaapcommon::fitters::SpectralFitter& fitter,
                                           gpu::Session& session,
                                           const ForcedTermImages* images) const;
  std::vector<float> FitTermsOnDevice(size_t scale_index, size_t n_terms,
                                      const DeviceFit& fit) const;
  /// The batched fit of a scale, its term-major result (n_terms rows of
  /// ComponentCount(scale_index) floats) left in d_terms on the device.
  void FitTermsIntoDevice(size_t scale_index, size_t n_terms, const DeviceFit& fit,
                          gpu::Buffer& d_terms) const;
  std::vector<float> FitTermsOnHost(size_t scale_index, size_t n_terms,
                                    const schaapcommon::fitters::SpectralFitter& fitter) const;
  void WriteRows(const std::string& filename,
                 const schaapcommon::fitters::SpectralFitter& fitter,
                 const std::vector<double>& scale_sizes, long double pixel_scale_x,
                 long double pixel_scale_y, long double phase_centre_ra,
                 long double phase_centre_dec, long double l_shift, long double m_shift,
                 gpu::Session* session, const ForcedTermImages* images) const;
  size_t width_ = 0, height_ = 0, n_frequencies_ = 0;
  size_t added_since_merge_ = 0;
  std::vector<ScaleList> list_per_scale_;
};

}  // namespace radler
