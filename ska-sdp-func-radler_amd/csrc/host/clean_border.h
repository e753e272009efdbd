// The border that the peak searches and the sub-minor loops leave unsearched
// at each side of an image: round(size * border ratio), the product formed in
// float and rounded half away from zero, and where a scale is given at least
// half the scale, rounded up (the box of
// ThreadedDeconvolutionTools::FindMultiScalePeak).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace radler::algorithms {

struct Borders {
  uint32_t horizontal, vertical;
};

inline uint32_t CleanBorder(size_t size, float ratio, float scale = 0.0f) {
  return uint32_t(
      std::max(size_t(std::round(size * ratio)), size_t(std::ceil(scale * 0.5))));
}

inline Borders CleanBorders(size_t width, size_t height, float ratio, float scale = 0.0f) {
  return {CleanBorder(width, ratio, scale), CleanBorder(height, ratio, scale)};
}

}  // namespace radler::algorithms
