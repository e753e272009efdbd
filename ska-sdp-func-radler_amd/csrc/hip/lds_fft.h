// Runtime-plan LDS FFT kernels (lds_fft.hip): the plan and the three pass
// launches used by the convolution object (conv.hip) for the sizes without a
// compile-time plan.
#pragma once

#include <cstddef>
#include <cstdint>

#include "lds_fft_plan.h"  // the planner and its constants

struct rdl_session;

namespace rdl {

struct LdsPlan {
  uint32_t n;       // transform length
  uint32_t n_pass;
  uint8_t radix[kFftMaxPasses];
  const void* tw;   // n twiddles exp(-2 pi i k / n), Cx<T>
};

/* The plan of a length-n transform (RDL_ERR_UNSUPPORTED unless n is
 * 2/3/5/7-smooth) and its twiddle table W_n^k, float or double complex,
 * hipMalloc'ed into *tw (the compile-time kernels read the same table). */
int MakeLdsPlan(rdl_session* s, uint32_t n, bool f64, LdsPlan* plan, void** tw);

/* The three passes over a plan.n-wide (rows) / plan.n-high (columns) plane,
 * `count` transforms per workgroup; spectra are row-major with width/2+1
 * columns, Cx<float> or Cx<double> by f64.
 * Rows forward: the img_w x img_h image at (ox, oy) of the plane, zero
 * elsewhere; row_mask (or NULL): per plane row, 0 = known zero. */
int LdsRowsForwardLaunch(rdl_session* s, const LdsPlan& plan, bool f64, uint32_t count,
                         uint32_t height, const float* in, uint32_t img_w, uint32_t img_h,
                         uint32_t ox, uint32_t oy, void* spec, const uint8_t* row_mask);
/* Rows inverse: the window is written to `out` (img_w wide) or subtracted. */
int LdsRowsInverseLaunch(rdl_session* s, const LdsPlan& plan, bool f64, uint32_t count,
                         uint32_t height, const void* spec, float* out, uint32_t img_w,
                         uint32_t img_h, uint32_t ox, uint32_t oy, int subtract);
/* Columns of a `width`-wide plane: mode 0 forward / 1 forward x K x s inverse /
 * 2 x K x s inverse; kern_cm: K column-major, out_cm (mode 0): so the output. */
int LdsColumnsLaunch(rdl_session* s, const LdsPlan& plan, bool f64, uint32_t count,
                     uint32_t width, const void* in, void* out, const void* kern, int mode,
                     double scale, const uint8_t* row_mask, int kern_cm, int out_cm);

/* The split (four-step) column passes: a column of length n1 * n2 as two
 * coalesced passes A and B (see SplitArgs in lds_fft.hip), `cols` adjacent
 * columns per tile. One launch is one pass over the whole spectrum; A: mode 0
 * forward, 1 inverse; B: mode 0 forward, 1 forward x K x s inverse, 2 x K x s
 * inverse. col_plan: the full-length plan (its twiddles, its length). */
struct LdsSplit {
  uint32_t n1, n2, cols;
  LdsPlan plan_n1, plan_n2;
};
int LdsColumnsSplitLaunch(rdl_session* s, const LdsSplit& sp, const LdsPlan& col_plan, bool f64,
                          uint32_t width, bool pass_b, int mode, const void* in, void* out,
                          const void* kern, double scale, const uint8_t* row_mask);

}  // namespace rdl
