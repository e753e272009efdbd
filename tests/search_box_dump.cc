// Reads lines of  w h start_y end_y h_border v_border  and prints
// rdl::MakeSearchBox (csrc/hip/conv_peak_box.h) for each:  xs xe ys ye
// tests/test_boxed_cases.py compares each line with boxed_cases.box.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "conv_peak_box.h"

int main() {
  uint32_t w, h, start_y, end_y, hb, vb;
  while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &w, &h,
                    &start_y, &end_y, &hb, &vb) == 6) {
    const rdl::PeakBox b = rdl::MakeSearchBox(w, h, start_y, end_y, hb, vb);
    std::printf("%u %u %u %u\n", b.xs, b.xe, b.ys, b.ye);
  }
  return 0;
}
