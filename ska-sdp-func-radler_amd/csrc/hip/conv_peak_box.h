// The search box of the peak searches fused into the inverse row pass
// (rdl_conv_rows_inverse_peak, rdl_conv_convolve_subtract_peak): the box of
// rdl_find_peak(start_y 0, end_y h) on a w x h image (peak_finder.cc:27-32).
// Host C++ only, so that a plain compiler can test it.
#pragma once

#include <cstdint>

namespace rdl {

struct PeakBox {
  uint32_t xs, xe, ys, ye;  // x in [xs, xe), y in [ys, ye); xs <= xe, ys <= ye
};

// [border, n - border), empty (end == start) when the borders meet or the
// border is wider than the image
inline uint32_t PeakBoxEnd(uint32_t n, uint32_t border) {
  return border <= n && n - border > border ? n - border : border;
}

inline PeakBox MakePeakBox(uint32_t w, uint32_t h, uint32_t h_border, uint32_t v_border) {
  return PeakBox{h_border, PeakBoxEnd(w, h_border), v_border, PeakBoxEnd(h, v_border)};
}

}  // namespace rdl
