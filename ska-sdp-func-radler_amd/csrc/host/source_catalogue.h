// radler::SourceCatalogue: a source catalogue read back from the text format
// ComponentList::Write emits (cpp/utils/write_model.h), and drawn into model
// images or restored onto residuals on the device: what WSClean does with
// -draw-model and -restore-list. WSClean's renderer is not part of the
// reference snapshot, so parity with it is unpinned; DESIGN.md ("Source
// catalogues") states the format accepted, the conventions and the contract.
//
// Conventions
//  * (ra, dec) -> (l, m) about the phase centre (ImageCoordinates::RaDecToLM),
//    minus the shifts, -> fractional pixels x = width/2 - l/pixel_scale_x,
//    y = height/2 + m/pixel_scale_y: the inverses of what Write applies, in
//    long double. Sources with l^2 + m^2 >= 1 or behind the phase centre are
//    dropped and counted.
//  * MajorAxis / MinorAxis are FWHM in arcsec, Orientation is in degrees: the
//    position angle of the major axis in restore.h's convention for beam_pa
//    (the major axis along (cos, sin)(pa + pi/2) in the (l, m) frame). The
//    covariance in (l, m) is mapped to pixels by
//    J = diag(-1/pixel_scale_x, 1/pixel_scale_y).
//  * S(nu): LogarithmicSI true is rdl::lp::Evaluate with I as term 0 and
//    lg = log10(nu / nu_ref); false is SpectralFitter::Evaluate's float
//    polynomial in x = nu / nu_ref - 1. A source without terms has I at every
//    frequency.
#pragma once

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "aocommon_compat.h"
#include "device.h"

namespace radler {

class SourceCatalogue {
 public:
  enum class Type { kPoint, kGaussian };
  struct Source {
    std::string name;
    Type type = Type::kPoint;
    long double ra = 0.0L, dec = 0.0L;  // radians
    float flux = 0.0f;                  // I: Jy at the reference frequency
    std::vector<float> terms;           // SpectralIndex: the terms after I
    bool logarithmic = true;            // LogarithmicSI
    double reference_frequency = 0.0;   // Hz; 0: none given (and no terms)
    double major = 0.0, minor = 0.0;    // FWHM, arcsec
    double orientation = 0.0;           // degrees
  };
  /// Where the catalogue is drawn: the image and its phase centre.
  struct Geometry {
    size_t width = 0, height = 0;
    long double pixel_scale_x = 0.0L, pixel_scale_y = 0.0L;  // radians
    long double phase_centre_ra = 0.0L, phase_centre_dec = 0.0L;
    long double l_shift = 0.0L, m_shift = 0.0L;
  };
  /// A clean beam: FWHM axes and position angle in radians (restore.h).
  struct Beam {
    long double major = 0.0L, minor = 0.0L, pa = 0.0L;
  };

  /// Parses a catalogue. Every malformed line throws std::runtime_error
  /// naming the file and the 1-based line number.
  static SourceCatalogue Read(const std::string& filename);

  size_t Size() const { return sources_.size(); }
  const std::vector<Source>& Sources() const { return sources_; }
  /// The header's ReferenceFrequency default; without one the first row's; 0
  /// when the file gives none.
  double ReferenceFrequency() const;
  /// The sources the last geometry call (PixelPositions, DrawModel, Restore)
  /// dropped: off the sky's near hemisphere as seen from its phase centre.
  size_t Dropped() const { return dropped_; }

  /// S(nu): n_freq rows of Size() floats.
  std::vector<float> FluxAt(const std::vector<double>& frequencies) const;
  /// Fractional pixel coordinates (x, y) of every source; NaNs for a dropped
  /// one.
  std::vector<std::pair<double, double>> PixelPositions(const Geometry& geometry) const;

  /// The catalogue as frequencies.size() zero-initialised model planes in
  /// Jy/pixel: a POINT (and a GAUSSIAN with an axis <= 0) adds S(nu) to its
  /// nearest pixel; a GAUSSIAN is drawn at its sub-pixel centre with integral
  /// S(nu), over the box ceil(6 sigma_major) pixels either side
  /// (rdl_draw_sources). Throws std::invalid_argument, before a device call,
  /// for an empty image, a pixel scale or frequency <= 0 and more than
  /// RDL_MAX_IMAGES frequencies.
  std::vector<aocommon::Image> DrawModel(gpu::Session& session, const Geometry& geometry,
                                         const std::vector<double>& frequencies) const;
  /// d_images (frequencies.size() contiguous width x height planes of the
  /// session) += every source convolved with the beam, in Jy/beam: drawn at
  /// its sub-pixel centre as the Gaussian of covariance source + beam, with
  /// peak S(nu) sqrt(det beam / det(source + beam)). Beam checks as
  /// radler::math::RestoreImage, but a beam with both axes 0 is refused too.
  void Restore(gpu::Session& session, float* d_images, const Geometry& geometry,
               const std::vector<double>& frequencies, const Beam& beam) const;
  /// The same two with the geometry and the beam spelled out.
  std::vector<aocommon::Image> DrawModel(gpu::Session& session, size_t width, size_t height,
                                         long double pixel_scale_x, long double pixel_scale_y,
                                         long double phase_centre_ra,
                                         long double phase_centre_dec,
                                         const std::vector<double>& frequencies,
                                         long double l_shift = 0.0L,
                                         long double m_shift = 0.0L) const {
    return DrawModel(session,
                     Geometry{width, height, pixel_scale_x, pixel_scale_y, phase_centre_ra,
                              phase_centre_dec, l_shift, m_shift},
                     frequencies);
  }
  void Restore(gpu::Session& session, float* d_images, size_t width, size_t height,
               long double pixel_scale_x, long double pixel_scale_y, long double phase_centre_ra,
               long double phase_centre_dec, const std::vector<double>& frequencies,
               long double beam_major, long double beam_minor, long double beam_pa,
               long double l_shift = 0.0L, long double m_shift = 0.0L) const {
    Restore(session, d_images,
            Geometry{width, height, pixel_scale_x, pixel_scale_y, phase_centre_ra,
                     phase_centre_dec, l_shift, m_shift},
            frequencies, Beam{beam_major, beam_minor, beam_pa});
  }
  /// The argument checks of DrawModel and (with a beam) Restore on their own.
  static void CheckArguments(const Geometry& geometry, const std::vector<double>& frequencies,
                             const Beam* beam);

  /// What rdl_draw_sources is given: the kept sources' shapes and, per
  /// frequency, their amplitudes (frequencies.size() rows of shapes.size()).
  struct Drawing {
    std::vector<rdl_source_shape> shapes;
    std::vector<float> amplitudes;
  };
  Drawing MakeDrawing(const Geometry& geometry, const std::vector<double>& frequencies,
                      const Beam* beam) const;

 private:
  std::vector<Source> sources_;
  double header_reference_frequency_ = 0.0;
  mutable size_t dropped_ = 0;
};

}  // namespace radler
