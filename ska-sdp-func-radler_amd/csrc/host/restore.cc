#include "restore.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "component_optimization.h"
#include "fft_sizes.h"

namespace radler::math {

RestoreKernel MakeRestoreKernel(size_t width, size_t height, long double beam_major,
                                long double beam_minor, long double beam_pa,
                                long double pixel_scale_l, long double pixel_scale_m) {
  const long double fwhm_to_sigma = 1.0L / (2.0L * sqrtl(2.0L * logl(2.0L)));
  const long double sigma_major = beam_major * fwhm_to_sigma;
  const long double sigma_minor = beam_minor * fwhm_to_sigma;
  const long double angle = beam_pa + 0.5L * M_PI;  // from North
  const double sigma_max = double(std::max(fabsl(sigma_major * cosl(angle)),
                                           fabsl(sigma_major * sinl(angle))));
  const size_t min_dim = std::min(width, height);
  size_t box = std::min<size_t>(
      size_t(std::ceil(sigma_max * 40.0 / double(std::min(pixel_scale_l, pixel_scale_m)))),
      min_dim);
  if (box % 2 != 0) ++box;
  if (box > min_dim) box = min_dim;
  return {double(sigma_major), double(sigma_minor), double(angle), box};
}

void RestoreImage(gpu::Session& s, float* d_image, const float* d_model, size_t width,
                  size_t height, long double beam_major, long double beam_minor,
                  long double beam_pa, long double pixel_scale_l, long double pixel_scale_m) {
  const size_t n = width * height;
  if (n == 0) return;
  if (beam_major == 0.0L && beam_minor == 0.0L) {
    gpu::Check(rdl_add(s.Handle(), d_image, d_model, n), "rdl_add");
    return;
  }
  if (!(beam_major > 0.0L) || !(beam_minor > 0.0L))
    throw std::invalid_argument("RestoreImage: a beam axis is not positive");
  if (!(pixel_scale_l > 0.0L) || !(pixel_scale_m > 0.0L))
    throw std::invalid_argument("RestoreImage: a pixel scale is not positive");
  const RestoreKernel k = MakeRestoreKernel(width, height, beam_major, beam_minor, beam_pa,
                                            pixel_scale_l, pixel_scale_m);
  if (k.box == 0) throw std::invalid_argument("RestoreImage: the beam is smaller than a pixel");
  // the image sits in the middle of the padded plane with at least box / 2
  // zeros on every side, the kernel's reach
  const size_t pw = utils::CalculateGoodFFTSize(width + k.box),
               ph = utils::CalculateGoodFFTSize(height + k.box), pn = pw * ph;
  gpu::Fft& fft = s.GetFft(pw, ph, true);
  // -G: the padded convolution the session has subtracts its result, and
  // image - float(model x -G) is image + float(model x G), bit for bit
  gpu::Buffer placed(s, pn * sizeof(float));
  gpu::Check(rdl_place_gaussian(s.Handle(), placed.F(), uint32_t(pw), uint32_t(ph),
                                uint32_t(k.box), double(pixel_scale_l), double(pixel_scale_m),
                                k.sigma_major, k.sigma_minor, k.angle),
             "rdl_place_gaussian");
  gpu::Check(rdl_scale(s.Handle(), placed.F(), pn, -1.0f), "rdl_scale");
  gpu::Buffer spectrum(s, fft.SpectrumBytes());
  if (fft.UsesLds()) {  // float in, float64 transforms
    fft.ForwardColumnMajor(placed.F(), spectrum.Ptr());
  } else {  // rocFFT double
    gpu::Buffer placed64(s, pn * sizeof(double));
    gpu::Check(rdl_convert(s.Handle(), placed.F(), placed64.D(), pn, 1), "rdl_convert");
    fft.Forward64(placed64.D(), spectrum.Ptr());
  }
  PaddedConvolveSubtract(s, d_model, d_image, width, height, pw, ph, spectrum.Ptr());
}

}  // namespace radler::math
