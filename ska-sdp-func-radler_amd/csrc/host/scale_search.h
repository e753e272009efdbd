// The parts that the peak searches over scale-convolved images share between
// MultiScaleAlgorithm and AspAlgorithm: storing the collected peaks, the two
// session lanes, and the two ways from an image to every scale's queued peak
// search (the fused multi-scale launch, or the full forward spectrum). Each
// algorithm chooses its source, its scales, its masks and its scale-0 search.
#pragma once

#include <memory>
#include <vector>

#include "clean_border.h"
#include "device.h"
#include "multiscale_algorithm.h"
#include "multiscale_transforms.h"

namespace radler::algorithms {

/// `transforms` made again unless it is bound to this session at this size
/// (another worker session runs the subimage when the ranks' ownership,
/// parallel_deconvolution.cc, changes between major iterations), then
/// planned for the largest of `plan_for`. Returns whether it was made.
bool EnsureTransforms(std::unique_ptr<multiscale::MultiScaleTransforms>& transforms,
                      gpu::Session& session, size_t width, size_t height, MultiscaleShape shape,
                      const std::vector<MultiScaleAlgorithm::ScaleInfo>* plan_for = nullptr);

/// A collected peak into its scale. normalized(value, x, y), the value over
/// the RMS factor at the peak (multiscale_algorithm.cc:736-743), is asked for
/// a found peak only.
template <class Normalized>
void StorePeak(MultiScaleAlgorithm::ScaleInfo& e, const rdl_peak& p, Normalized&& normalized) {
  e.max_image_value_x = p.x;
  e.max_image_value_y = p.y;
  e.max_unnormalized_image_value = p.found ? p.value : 0.0f;
  e.max_normalized_image_value = p.found ? normalized(p.value, p.x, p.y) : 0.0f;
}

/// One read for the queued searches of slots 0 .. pending.size() - 1: the
/// peak of slot k into scales[pending[k]].
template <class Normalized>
void CollectPeaks(rdl_session* s, const std::vector<size_t>& pending,
                  std::vector<MultiScaleAlgorithm::ScaleInfo>& scales,
                  Normalized&& normalized) {
  std::vector<rdl_peak> peaks(pending.size());
  gpu::Check(rdl_find_peak_collect(s, uint32_t(pending.size()), peaks.data()),
             "rdl_find_peak_collect");
  for (size_t k = 0; k != pending.size(); ++k)
    StorePeak(scales[pending[k]], peaks[k], normalized);
}

/// The session's two lanes under a run of independent steps: after Fork the
/// steps alternate over the lanes, until Join. Joins too when an exception
/// leaves the scope while forked.
class LanePair {
 public:
  explicit LanePair(rdl_session* s) : s_(s) {}
  LanePair(const LanePair&) = delete;
  ~LanePair() {
    if (forked_) (void)rdl_session_join(s_);
  }
  void Fork() {
    gpu::Check(rdl_session_fork(s_), "rdl_session_fork");
    forked_ = true;
  }
  /// selects the lane of the next step and returns it (lane 0 unless forked)
  int Select() {
    if (forked_) gpu::Check(rdl_session_lane(s_, lane_), "rdl_session_lane");
    return lane_;
  }
  void Advance() {
    if (forked_) lane_ ^= 1;
  }
  void Join() {
    if (!forked_) return;
    forked_ = false;
    lane_ = 0;
    gpu::Check(rdl_session_join(s_), "rdl_session_join");
  }

 private:
  rdl_session* s_;
  bool forked_ = false;
  int lane_ = 0;
};

/// One scale > 0 of a search.
struct ConvolvedScale {
  size_t index;  // in the algorithm's scale list
  float scale;
  float* d_image;  // W x H: takes the convolved image
  const uint8_t* d_mask;
  Borders border;
  float* rms = nullptr;  // takes the convolved image's RMS where it is reported
};

/// Queues the convolution and the peak search of every scale in `scales`, the
/// search of scales[k] in peak slot pending.size() + k, and appends the
/// scales' indices to `pending`. Two lanes (d_work[1] given) only where every
/// scale has an image of its own.
struct ScaleSearch {
  gpu::Session& session;
  multiscale::MultiScaleTransforms& transforms;
  void* d_spectrum;
  void* d_work[2];  // a spectrum-sized work buffer per lane
  std::vector<std::shared_ptr<gpu::Buffer>>& scale_u;  // Fused's inner inverses, grown here
  bool allow_negative;

  /// The scales' convolutions made from ONE forward half by one launch
  /// (rdl_conv_scales: the forward spectrum never reaches HBM, the scale
  /// kernels are real), then per scale the outer inverse step and the inverse
  /// rows with the fused peak search. Needs transforms.Fused().
  void Fused(const float* d_source, const std::vector<ConvolvedScale>& scales, bool two_lanes,
             std::vector<size_t>& pending);

  /// One forward spectrum, then per scale the product with the kernel
  /// spectrum and the inverse, with the peak search fused into the inverse
  /// row pass where `fused_peak` allows it and the plan has that form.
  /// Otherwise the search is queued over search_input(image): the image, or
  /// the RMS-weighted copy, which is why that search stays separate.
  template <class SearchInput>
  void ThroughSpectrum(const float* d_source, const std::vector<ConvolvedScale>& scales,
                       bool fused_peak, bool two_lanes, std::vector<size_t>& pending,
                       SearchInput&& search_input) {
    rdl_session* s = session.Handle();
    const size_t w = transforms.Width(), h = transforms.Height();
    transforms.Forward(d_source, d_spectrum);
    // The scales' inverse transforms + fused peak searches are independent
    // (the reference runs them on threads, threaded_deconvolution_tools.cc):
    // they alternate over two session lanes, so one scale's latency-bound row
    // pass overlaps the next one's column passes. Every buffer a lane writes
    // is its own (work spectrum, four-step scratch, peak partials slot, scale
    // image); the kernel spectra are made before the fork (no allocation on
    // lane 1).
    LanePair lanes(s);
    if (two_lanes) {
      for (const ConvolvedScale& c : scales) transforms.KernelSpectrum(c.scale);
      lanes.Fork();
    }
    for (const ConvolvedScale& c : scales) {
      const uint32_t slot = uint32_t(pending.size());
      pending.push_back(c.index);
      if (fused_peak &&
          transforms.ConvolveSpectrumPeak(d_spectrum, c.scale, d_work[lanes.Select()], c.d_image,
                                          c.border.horizontal, c.border.vertical,
                                          allow_negative, c.d_mask, slot)) {
        lanes.Advance();
        continue;
      }
      // no fused kernels for this size (nothing was issued): lane 0 from here
      lanes.Join();
      transforms.ConvolveSpectrum(d_spectrum, c.scale, d_work[0], c.d_image);
      if (c.rms) gpu::Check(rdl_rms(s, c.d_image, w * h, c.rms), "rdl_rms");
      // the scales' searches queue back to back; one read collects them
      gpu::Check(rdl_find_peak_enqueue(s, search_input(c.d_image), uint32_t(w), uint32_t(h), 0,
                                       uint32_t(h), c.border.horizontal, c.border.vertical,
                                       allow_negative, c.d_mask, 1, slot),
                 "rdl_find_peak_enqueue");
    }
    lanes.Join();
  }
};

}  // namespace radler::algorithms
