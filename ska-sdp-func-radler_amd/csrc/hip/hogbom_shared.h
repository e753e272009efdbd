// What the Högbom loops of clean.hip (one image set, two launches per
// component) and clean_batch.hip (one workgroup per plane) share: the
// subtraction window and the loop state kept in device memory.
#pragma once

#include "rdl_internal.h"

namespace rdl {

struct Window {
  uint32_t x0, x1, y0, y1;  // image coordinates, half-open
  int32_t off_x, off_y;     // psf(x - off_x, y - off_y)
};

__host__ __device__ inline Window SubtractWindow(uint32_t width,
                                                 uint32_t height, uint32_t x,
                                                 uint32_t y) {
  Window w;
  w.off_x = int32_t(x) - int32_t(width / 2);
  w.off_y = int32_t(y) - int32_t(height / 2);
  w.x0 = w.off_x > 0 ? uint32_t(w.off_x) : 0u;
  w.y0 = w.off_y > 0 ? uint32_t(w.off_y) : 0u;
  w.x1 = x + width / 2;
  if (w.x1 > width) w.x1 = width;
  w.y1 = y + height / 2;
  if (w.y1 > height) w.y1 = height;
  return w;
}

struct HogbomState {
  uint64_t iteration;
  uint64_t first_iteration;
  uint32_t done;
  uint32_t peak_index;
  float peak_value;
  int32_t found;
  int32_t diverging;
  uint32_t pad;
  float factors[RDL_MAX_IMAGES];
};

}  // namespace rdl
