// The restored image of a deconvolution on the device: residual + model
// convolved with the clean beam, what schaapcommon::math::RestoreImage does
// for WSClean. schaapcommon's source is not part of the reference snapshot,
// so its bit-level behaviour is unpinned; this file fixes the contract.
//
// The beam kernel G is rdl_place_gaussian's (rdl_hip.h): a box x box Gaussian
// of peak 1 (the restored image is in Jy/beam) with
//  * sigma = FWHM / (2 sqrt(2 ln 2)) for the major and the minor axis,
//  * the major axis at angle = beam_pa + pi/2 in rdl_place_gaussian's (l, m)
//    frame (l grows towards -x, m towards +y, each scaled by its pixel scale),
//  * box = ceil(40 sigma_max / min(pixel_scale_l, pixel_scale_m)), with
//    sigma_max = max(|sigma_major cos(angle)|, |sigma_major sin(angle)|), made
//    even and clipped to the smaller image side,
// the conventions the local-RMS window already uses (rms_image.cc).
//
// The convolution is linear, not circular: the model is zero-padded to
// CalculateGoodFFTSize(side + box) per axis, convolved and trimmed
// (schaapcommon's PaddedConvolution, as component_optimization.cc), so a
// source at an edge does not reappear at the opposite one. The transforms run
// in float64 and the result is rounded to float once, then added: a float32
// transform's noise, 2.5e-7 of the brightest source, is at the level of a deep
// residual (the same choice as rms_image.cc's window).
#pragma once

#include <cstddef>

#include "device.h"

namespace radler::math {

/// The beam kernel's geometry: rdl_place_gaussian's arguments.
struct RestoreKernel {
  double sigma_major = 0.0, sigma_minor = 0.0;  // in the units of the pixel scales
  double angle = 0.0;                           // beam_pa + pi/2
  size_t box = 0;                               // even, <= min(width, height)
};
RestoreKernel MakeRestoreKernel(size_t width, size_t height, long double beam_major,
                                long double beam_minor, long double beam_pa,
                                long double pixel_scale_l, long double pixel_scale_m);

/// d_image += d_model convolved with G (both width x height planes of the
/// session; they may not overlap). Beam axes (FWHM), position angle and pixel
/// scales in radians. beam_major == beam_minor == 0: d_image += d_model. Any
/// other beam with an axis <= 0, and a pixel scale <= 0, throw
/// std::invalid_argument before anything is launched.
void RestoreImage(gpu::Session& s, float* d_image, const float* d_model, size_t width,
                  size_t height, long double beam_major, long double beam_minor,
                  long double beam_pa, long double pixel_scale_l, long double pixel_scale_m);

}  // namespace radler::math
