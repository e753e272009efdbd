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

namespace rdl {

// The box of rdl_find_peak on a w x h image: peak_finder.cc:27-32 with its
// start_y / end_y, intersected with the image. The reference's unsigned bounds
// wrap when a border or start_y lies beyond the image; here every bound is
// clamped to the image first (the wrapped ends too) and an end below its start
// is then raised to it, so xs <= xe <= w and ys <= ye <= h for every input:
// ye - ys cannot wrap, and neither can xs + threadIdx.x (w + 255 < 2^32).
inline PeakBox MakeSearchBox(uint32_t w, uint32_t h, uint32_t start_y, uint32_t end_y,
                             uint32_t h_border, uint32_t v_border) {
  PeakBox b;
  b.xs = h_border;
  b.xe = w - h_border;
  b.ys = start_y > v_border ? start_y : v_border;
  b.ye = end_y < h - v_border ? end_y : h - v_border;
  if (b.xs > w) b.xs = w;
  if (b.ys > h) b.ys = h;
  if (b.xe > w) b.xe = w;
  if (b.ye > h) b.ye = h;
  if (b.xe < b.xs) b.xe = b.xs;
  if (b.ye < b.ys) b.ye = b.ys;
  return b;
}

}  // namespace rdl
