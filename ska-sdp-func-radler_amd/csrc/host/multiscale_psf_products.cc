// Line references are to the reference's
// cpp/algorithms/multiscale_algorithm.cc.
#include "multiscale_psf_products.h"

#include <iterator>

#include "host_profile.h"
#include "subminor.h"

namespace radler::algorithms {

bool MultiScalePsfProducts::Hit(const Inputs& in) const {
  if (session_ != &in.session || width_ != in.width || height_ != in.height ||
      n_psf_ != in.n_psf || !reference_.buffer || convolved_.size() != in.n_psf ||
      scales_ != in.scales || shape_ != in.shape ||
      convolution_padding_ != in.convolution_padding ||
      correction_f64_ != SubMinorLoop::CorrectionF64() ||
      correction_kernel_f32_ != SubMinorLoop::CorrectionKernelF32())
    return false;
  // The PSFs by content: Radler::Perform loads every major iteration's PSFs
  // into the same buffers, so their addresses say nothing.
  prof::Section prof_check("ms.psf_cache_check");
  rdl_session* s = in.session.Handle();
  const size_t plane_bytes = width_ * height_ * sizeof(float);
  gpu::Check(rdl_bits_differ_enqueue(s, in.d_integrated_psf, reference_.Plane(0), plane_bytes, 1),
             "rdl_bits_differ_enqueue");
  for (size_t i = 0; i != n_psf_; ++i)
    gpu::Check(rdl_bits_differ_enqueue(s, in.psfs.Plane(i), reference_.Plane(1 + i), plane_bytes,
                                       0),
               "rdl_bits_differ_enqueue");
  int differ = 1;
  gpu::Check(rdl_bits_differ_collect(s, &differ), "rdl_bits_differ_collect");
  return differ == 0;
}

bool MultiScalePsfProducts::ConvolvePsfs(const Inputs& in, bool keep,
                                         size_t budget) {  // :29-88
  prof::Section prof_psfs("ms.convolve_psfs");
  *this = MultiScalePsfProducts();
  session_ = &in.session;
  width_ = in.width;
  height_ = in.height;
  n_psf_ = in.n_psf;
  scales_ = in.scales;
  shape_ = in.shape;
  convolution_padding_ = in.convolution_padding;
  correction_f64_ = SubMinorLoop::CorrectionF64();
  correction_kernel_f32_ = SubMinorLoop::CorrectionKernelF32();
  const size_t n_scales = scales_.size();
  const size_t plane_bytes = width_ * height_ * sizeof(float);
  psf_peak_.assign(n_scales, 0.0f);
  convolved_.resize(n_psf_);
  auto convolve = [&](gpu::Planes& out, const float* d_psf, bool is_integrated) {
    out = gpu::Planes::Make(in.session, width_, height_, n_scales);
    for (size_t si = 0; si != n_scales; ++si) {
      in.session.D2D(out.Plane(si), d_psf, plane_bytes);
      if (scales_[si] != 0.0f) in.transforms.Transform(out.Plane(si), scales_[si]);
      if (is_integrated)
        psf_peak_[si] =
            in.session.ReadFloat(out.Plane(si) + width_ / 2 + (height_ / 2) * width_);
    }
  };
  convolve(convolved_[0], in.d_integrated_psf, true);
  if (n_psf_ > 1)
    for (size_t i = 0; i != n_psf_; ++i) convolve(convolved_[i], in.psfs.Plane(i), false);
  // kept only whole: the convolved PSFs and the copies the next major
  // iteration's PSFs are compared with
  const size_t set_bytes = (n_psf_ * n_scales + n_psf_ + 1) * plane_bytes;
  if (!keep || set_bytes > budget) return false;
  bytes_ = set_bytes;
  reference_ = gpu::Planes::Make(in.session, width_, height_, n_psf_ + 1);
  in.session.D2D(reference_.Plane(0), in.d_integrated_psf, plane_bytes);
  for (size_t i = 0; i != n_psf_; ++i)
    in.session.D2D(reference_.Plane(1 + i), in.psfs.Plane(i), plane_bytes);
  return true;
}

void MultiScalePsfProducts::Begin(const Inputs& in, bool keep, size_t budget) {
  if (!(keep && Hit(in))) keep = ConvolvePsfs(in, keep, budget);
  transforms_ = &in.transforms;
  keep_ = keep;
  budget_ = budget;
}

void MultiScalePsfProducts::End() {
  if (!keep_) {
    *this = MultiScalePsfProducts();
    return;
  }
  for (auto it = later_.begin(); it != later_.end();)
    it = it->second.kept ? std::next(it) : later_.erase(it);
}

bool MultiScalePsfProducts::Keeps(size_t bytes) {
  if (!keep_ || bytes_ + bytes > budget_) return false;
  bytes_ += bytes;
  return true;
}

const gpu::Planes& MultiScalePsfProducts::Twice(size_t scale) {  // :331-350
  const auto key = std::make_pair(kAllPsfs, scale);
  auto it = later_.find(key);
  if (it == later_.end()) {
    prof::Section prof_twice("ms.twice_convolved");
    const size_t plane_bytes = width_ * height_ * sizeof(float);
    gpu::Planes t = gpu::Planes::Make(*session_, width_, height_, n_psf_);
    for (size_t i = 0; i != n_psf_; ++i) {
      session_->D2D(t.Plane(i), convolved_[i].Plane(scale), plane_bytes);
      if (scales_[scale] != 0.0f) transforms_->Transform(t.Plane(i), scales_[scale]);
    }
    it = later_.emplace(key, Later{std::move(t), nullptr, Keeps(n_psf_ * plane_bytes)}).first;
  }
  return it->second.planes;
}

const gpu::Buffer& MultiScalePsfProducts::PaddedSpectrum(size_t psf, size_t scale, size_t conv_w,
                                                         size_t conv_h) {
  const auto key = std::make_pair(psf, scale);
  auto it = later_.find(key);
  if (it == later_.end()) {
    std::shared_ptr<gpu::Buffer> made = SubMinorLoop::MakeCorrectionPsfSpectrum(
        *session_, convolved_[psf].Plane(scale), width_, height_, conv_w, conv_h);
    const bool kept = Keeps(made->Bytes());
    it = later_.emplace(key, Later{gpu::Planes(), std::move(made), kept}).first;
  }
  return *it->second.buffer;
}

}  // namespace radler::algorithms
