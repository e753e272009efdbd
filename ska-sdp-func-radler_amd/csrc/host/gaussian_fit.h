// Elliptical Gaussian fitting and deconvolution for the adaptive-scale-pixel
// algorithm: the functions the reference takes from schaapcommon
// (fitters/gaussianfitter.h, math/ellipse.h; asp_algorithm.cc:72-73, 267-269,
// 277-278). schaapcommon's source is not part of the reference snapshot, so
// their bit-level behaviour is unpinned; this file fixes the contracts.
//
// The Gaussian and its position-angle convention are rdl_hip.h's ("adaptive
// scale pixel"). The fits are Levenberg-Marquardt in host double over the
// device sums of rdl_gaussian_fit_sums, one 224-byte read per evaluation.
//
// The rules (tests/asp_lib.py restates them in numpy float64):
//  * lambda starts at 1e-3. A step solves (N + lambda diag(N)) delta = J^T r
//    over the free parameters (Marquardt's diagonal scaling), N = J^T J; a
//    fixed parameter's row and column are dropped, and so is, for that step,
//    a free parameter whose diagonal element is zero.
//  * The trial p + delta is rejected without an evaluation when a value is
//    non-finite or a FWHM is not positive. Otherwise it is evaluated and
//    accepted when its sum of squares is strictly smaller.
//  * Accepted: lambda = max(lambda / 10, 1e-12). The fit stops when
//    max_i |delta_i| / max(|p_i|, 1) < 1e-10 or the sum of squares fell by no
//    more than 1e-14 of its value.
//  * Rejected (or the system is singular): lambda *= 10; the fit stops when
//    lambda exceeds 1e12.
//  * At most 100 evaluations of the sums per fit, the first included.
//  * After a fit: major >= minor (swapped with pa += pi/2 otherwise) and pa
//    folded into [-pi/2, pi/2).
#pragma once

#include <cstddef>

#include "device.h"

namespace schaapcommon::math {
struct Ellipse {
  double major = 0.0;           // FWHM, pixels
  double minor = 0.0;           // FWHM, pixels
  double position_angle = 0.0;  // radians, from +x towards +y
};
}  // namespace schaapcommon::math

namespace schaapcommon::fitters {

constexpr double kLmLambdaStart = 1e-3;
constexpr double kLmLambdaMin = 1e-12;
constexpr double kLmLambdaMax = 1e12;
constexpr double kLmStepTolerance = 1e-10;
constexpr double kLmDecreaseTolerance = 1e-14;
constexpr size_t kLmMaxEvaluations = 100;
constexpr size_t kFitMaxRounds = 5;

/// Fits amplitude, position and shape (all six parameters, in/out) to the
/// width x height device image. The fitting box is square, of side
/// max(10, ceil(10 major)) made even, centred on the rounded position and
/// clipped to the image; the fit is repeated with the new box while the side
/// changes, at most 5 rounds. A box that covers the image gives one fit over
/// the whole image.
void Fit2DGaussianFull(radler::gpu::Session& s, const float* d_image, size_t width,
                       size_t height, double& amplitude, double& x, double& y,
                       double& major, double& minor, double& position_angle);

/// Fits the shape of a Gaussian whose centre is fixed at (width/2, height/2)
/// and whose amplitude is fixed at that pixel's value, starting from a
/// circular one of FWHM beam_estimate; the box rule of Fit2DGaussianFull.
math::Ellipse Fit2DGaussianCentred(radler::gpu::Session& s, const float* d_image,
                                   size_t width, size_t height, double beam_estimate);

/// The ellipse that, convolved with `psf`, gives `ellipse`: the second-moment
/// matrices subtract. All three members are NaN when the difference is not
/// positive definite (the ellipse is not larger than the PSF along every
/// direction). Pure host function.
math::Ellipse DeconvolveGaussian(const math::Ellipse& ellipse, const math::Ellipse& psf);

}  // namespace schaapcommon::fitters
