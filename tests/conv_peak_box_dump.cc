// Prints rdl::MakePeakBox (csrc/hip/conv_peak_box.h) over small images and
// every border up to two past the image side, and the widest border:
//   w h h_border v_border xs xe ys ye
// tests/test_conv_peak_box.py compares each line with the closed form.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "conv_peak_box.h"

int main() {
  std::vector<uint32_t> sides{0, 1, 2, 3, 4, 5, 6};
  auto borders = [](uint32_t n) {
    std::vector<uint32_t> b;
    for (uint32_t i = 0; i <= n + 2; ++i) b.push_back(i);
    b.push_back(0xffffffffu);
    return b;
  };
  auto dump = [&](uint32_t w, uint32_t h) {
    for (uint32_t hb : borders(w))
      for (uint32_t vb : borders(h)) {
        const rdl::PeakBox b = rdl::MakePeakBox(w, h, hb, vb);
        std::printf("%u %u %u %u %u %u %u %u\n", w, h, hb, vb, b.xs, b.xe, b.ys, b.ye);
      }
  };
  for (uint32_t w : sides)
    for (uint32_t h : sides) dump(w, h);
  dump(64, 48);
  return 0;
}
