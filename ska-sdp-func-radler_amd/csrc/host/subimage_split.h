// The subimage geometry of a gridded run (reference's :34-166); host code only.
#pragma once

#include <cstddef>
#include <vector>

#include "psf_offset.h"
#include "settings.h"

namespace radler::algorithms {

/// One tile of the grid (parallel_deconvolution.h SubImage).
struct SubImage {
  size_t index = 0, x = 0, y = 0, width = 0, height = 0;
  std::vector<bool> mask, boundary_mask;
  double peak = 0.0;
  bool reached_major_threshold = false;
};

/// Subimage geometry of the grid (parallel_deconvolution.cc:57-166).
std::vector<SubImage> MakeSubImages(const std::vector<float>& image, size_t width,
                                    size_t height, const bool* user_mask,
                                    const std::vector<PsfOffset>& psf_offsets,
                                    const Settings& settings,
                                    std::vector<size_t>& psf_indices);

/// parallel_deconvolution.cc:34-55 (first index on equal distance).
size_t NearestPsfIndex(const std::vector<PsfOffset>& psf_offsets, size_t x,
                       size_t y) noexcept;

}  // namespace radler::algorithms
