#include "scale_search.h"

#include <algorithm>

namespace radler::algorithms {

using multiscale::MultiScaleTransforms;

bool EnsureTransforms(std::unique_ptr<MultiScaleTransforms>& transforms, gpu::Session& session,
                      size_t width, size_t height, MultiscaleShape shape,
                      const std::vector<MultiScaleAlgorithm::ScaleInfo>* plan_for) {
  const bool make = !transforms || !transforms->BoundTo(session) ||
                    transforms->Width() != width || transforms->Height() != height;
  if (make) transforms = std::make_unique<MultiScaleTransforms>(session, width, height, shape);
  if (plan_for) {
    float max_scale = 0.0f;
    for (const MultiScaleAlgorithm::ScaleInfo& e : *plan_for)
      max_scale = std::max(max_scale, e.scale);
    transforms->SetMaxScale(max_scale);
  }
  return make;
}

void ScaleSearch::Fused(const float* d_source, const std::vector<ConvolvedScale>& scales,
                        bool two_lanes, std::vector<size_t>& pending) {
  // every buffer and kernel spectrum before any fork (no allocation on lane 1)
  const size_t spectrum_bytes = transforms.SpectrumBytes();
  while (scale_u.size() < scales.size())
    scale_u.push_back(std::make_shared<gpu::Buffer>(session, spectrum_bytes));
  std::vector<float> sizes;
  std::vector<void*> outs;
  for (size_t k = 0; k != scales.size(); ++k) {
    sizes.push_back(scales[k].scale);
    outs.push_back(scale_u[k]->Ptr());
  }
  for (float size : sizes) transforms.RealKernelSpectrum(size);
  transforms.ForwardHalf(d_source, d_spectrum);
  transforms.Scales(d_spectrum, sizes, outs);
  LanePair lanes(session.Handle());
  if (two_lanes) lanes.Fork();
  for (size_t k = 0; k != scales.size(); ++k) {
    const ConvolvedScale& c = scales[k];
    transforms.FinishPeak(outs[k], c.scale, d_work[lanes.Select()], c.d_image,
                          c.border.horizontal, c.border.vertical, allow_negative, c.d_mask,
                          uint32_t(pending.size()));
    pending.push_back(c.index);
    lanes.Advance();
  }
  lanes.Join();
}

}  // namespace radler::algorithms
