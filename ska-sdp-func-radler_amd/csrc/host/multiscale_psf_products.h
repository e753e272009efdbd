// The PSF-derived products of a multiscale major iteration: the
// scale-convolved PSFs with the scales' PSF peaks (ConvolvePsfs,
// multiscale_algorithm.cc:29-88), and, made when first used, the
// twice-convolved PSFs of a scale (:331-350) and the padded spectra of the
// convolved PSFs that the residual correction multiplies with.
//
// On a main session they are kept for the next major iteration while the
// PSFs, the scales and the sizes stay the same (the PSF of a deconvolution
// does not change between its major iterations) and while they fit the
// budget. A kept product is the product that would be made again from the
// same inputs by the same kernels. A worker session's clones and
// RDL_PSF_CACHE=0 keep nothing past the major iteration's return.
#pragma once

#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "device.h"
#include "multiscale_transforms.h"
#include "settings.h"

namespace radler::algorithms {

class MultiScalePsfProducts {
 public:
  /// what the products are made from
  struct Inputs {
    gpu::Session& session;
    multiscale::MultiScaleTransforms& transforms;
    size_t width, height;
    const std::vector<float>& scales;
    MultiscaleShape shape;
    double convolution_padding;
    size_t n_psf;
    const float* d_integrated_psf;
    const gpu::Planes& psfs;
  };

  /// Erases, when the major iteration returns, the products that are not
  /// kept past it. Made before Begin.
  struct IterationGuard {
    MultiScalePsfProducts& products;
    ~IterationGuard() { products.End(); }
  };

  /// The products of `in` for this major iteration: the kept ones if they were
  /// made from the same inputs (the PSFs compared by content on the device),
  /// else the convolved PSFs made again. With `keep` they may stay past the
  /// return within `budget` bytes: the convolved PSFs with the copies the next
  /// PSFs are compared with only whole, at (n_psf * n_scales + n_psf + 1)
  /// planes, and with them every later product that still fits when it is
  /// made. in.transforms makes the later products, until End.
  void Begin(const Inputs& in, bool keep, size_t budget);

  float PsfPeak(size_t scale) const { return psf_peak_[scale]; }
  /// [scale] of the PSF `psf`; with one PSF, of the integrated PSF
  const gpu::Planes& Convolved(size_t psf) const { return convolved_[psf]; }
  /// [psf] of the scale, convolved with it twice. The reference stays valid
  /// until End, as PaddedSpectrum's does.
  const gpu::Planes& Twice(size_t scale);
  /// the conv_w x conv_h correction spectrum of Convolved(psf).Plane(scale)
  const gpu::Buffer& PaddedSpectrum(size_t psf, size_t scale, size_t conv_w, size_t conv_h);

 private:
  /// whether the products are those of `in`: the cheap fields, then the
  /// content comparison (queued and waited for)
  bool Hit(const Inputs& in) const;
  /// makes the convolved PSFs; returns whether they are kept past End
  bool ConvolvePsfs(const Inputs& in, bool keep, size_t budget);
  void End();
  /// counts a product made now against the budget; false: it goes at End
  bool Keeps(size_t bytes);

  // the key: everything the products depend on; the PSFs by content
  // (`reference_`: the integrated PSF, then every PSF plane, compared bit for
  // bit on the device)
  gpu::Session* session_ = nullptr;
  size_t width_ = 0, height_ = 0, n_psf_ = 0;
  std::vector<float> scales_;
  MultiscaleShape shape_{};
  double convolution_padding_ = 0.0;
  bool correction_f64_ = true, correction_kernel_f32_ = false;
  gpu::Planes reference_;

  std::vector<float> psf_peak_;         // per scale
  std::vector<gpu::Planes> convolved_;  // [psf][scale]
  // made when first used: (kAllPsfs, scale) the twice-convolved PSFs,
  // (psf, scale) a padded spectrum
  static constexpr size_t kAllPsfs = ~size_t{0};
  struct Later {
    gpu::Planes planes;                  // twice-convolved
    std::shared_ptr<gpu::Buffer> buffer;  // padded spectrum
    bool kept;                           // past End
  };
  std::map<std::pair<size_t, size_t>, Later> later_;

  // this major iteration
  multiscale::MultiScaleTransforms* transforms_ = nullptr;
  bool keep_ = false;
  size_t budget_ = 0;
  size_t bytes_ = 0;  // held by the kept products
};

}  // namespace radler::algorithms
