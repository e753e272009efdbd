// Prints radler::algorithms::CleanBorders (csrc/host/clean_border.h), which
// DeconvolutionAlgorithm::PeakBorders calls with its border ratio, over
// mixed image sides, border ratios and scales:
//   width height ratio_index scale_index horizontal vertical
// tests/test_clean_border.py compares each line with the closed form.
#include <cstddef>
#include <cstdio>

#include "clean_border.h"

int main() {
  const size_t sides[] = {1, 2, 3, 64, 100, 1000, 8192};
  const float ratios[] = {0.0f, 0.01f, 0.05f, 0.125f, 0.25f, 0.5f};
  const float scales[] = {0.0f, 1.0f, 4.5f, 5.0f, 37.2f, 300.0f};
  for (size_t w : sides)
    for (size_t h : sides)
      for (int r = 0; r != 6; ++r)
        for (int s = 0; s != 6; ++s) {
          const radler::algorithms::Borders b =
              radler::algorithms::CleanBorders(w, h, ratios[r], scales[s]);
          std::printf("%zu %zu %d %d %u %u\n", w, h, r, s, b.horizontal, b.vertical);
        }
  return 0;
}
