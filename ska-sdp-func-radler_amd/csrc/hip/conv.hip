// The rdl_conv object and every rdl_conv_* entry point: a width x height
// real 2-D transform pair as three HBM passes (rows / columns / rows, see
// lds_fft.hip). Each pass picks, per call, the tiled four-step plans or the
// compile-time plans of fft_fast*.hip where the size has one, and the
// runtime-plan kernels of lds_fft.hip elsewhere. No kernel lives here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "conv_peak_box.h"
#include "fft_fast.h"
#include "lds_fft.h"
#include "rdl_internal.h"

struct rdl_conv {
  rdl_session* s = nullptr;
  uint32_t width = 0, height = 0;
  bool f64 = false;
  void* tw_row = nullptr;
  void* tw_col = nullptr;
  rdl::LdsPlan row_plan{}, col_plan{};
  uint32_t row_count = 1, col_count = 1;
  // split (four-step) column passes of the runtime plans (rdl_conv_create_ex)
  bool split = false;
  rdl::LdsSplit sp{};
  void* tw_n1 = nullptr;
  void* tw_n2 = nullptr;
  // spectrum-sized, for the out-of-place four-step passes; one per session lane
  void* scratch_lane[2] = {nullptr, nullptr};
  void* scratch = nullptr;  // the current lane's (set by EnsureLaneScratch)
  size_t scratch_bytes[2] = {0, 0};
  // compile-time-planned kernels (fft_fast*.hip) where the size has a plan
  const rdl::FastColumns* fast_cols = nullptr;
  const rdl::FastColumns* conv_cols = nullptr;  // float64 mode-1 columns (ColumnsConvD)
  const rdl::FastRows* fast_rows = nullptr;
  uint32_t* rows_list = nullptr;            // height words + the count
  const uint8_t* rows_list_mask = nullptr;  // mask the list was made from
  // float planes with four-step column plans: spectra in 16-column tiles
  const rdl::FastSteps* steps = nullptr;
  bool tiled = false;
  // pass tables of the compile-time plans (rdl::MakePassTable)
  void* ptw_row = nullptr;
  void* ptw_col = nullptr;
  void* ptw_a = nullptr;
  void* ptw_b = nullptr;
  void* twd_row = nullptr;  // float rows: two-level double twiddles of width (MakeTwiddleBase)
  // rdl_conv_real_kernel: cosine tables of width and height, stage-1 scratch
  void* cos_w = nullptr;
  void* cos_h = nullptr;
  rdl::Scratch real_a;
};

namespace {

double SpectrumBytes(const rdl_conv* c) {
  if (c->tiled) return double(rdl::TiledComplexCount(c->width, c->height)) * 8.0;
  return double(c->width / 2 + 1) * c->height * (c->f64 ? 16.0 : 8.0);
}

// the current lane's spectrum-sized scratch, in c->scratch
int EnsureLaneScratch(rdl_conv* c, size_t bytes) {
  const int l = c->s->lane;
  c->scratch = c->scratch_lane[l];
  if (c->scratch_bytes[l] >= bytes) return RDL_OK;
  if (c->scratch) {
    RDL_HIP_CHECK(hipStreamSynchronize(c->s->home));
    if (c->s->aux) RDL_HIP_CHECK(hipStreamSynchronize(c->s->aux));
    RDL_HIP_CHECK(rdl::DevFree(c->scratch));
    c->scratch = c->scratch_lane[l] = nullptr;
    c->scratch_bytes[l] = 0;
  }
  RDL_HIP_CHECK(rdl::DevMalloc(&c->scratch, bytes));
  if (rdl::PoisonOn()) RDL_HIP_CHECK(hipMemsetAsync(c->scratch, 0xff, bytes, c->s->stream));
  c->scratch_lane[l] = c->scratch;
  c->scratch_bytes[l] = bytes;
  return RDL_OK;
}

// the non-zero rows of `row_mask` as a device list (+ count), made once per
// rows-forward / columns pair
int CompactRowsFor(rdl_conv* c, const uint8_t* row_mask, bool reuse) {
  if (reuse && c->rows_list_mask == row_mask) return RDL_OK;
  if (!c->rows_list)
    RDL_HIP_CHECK(rdl::DevMalloc(&c->rows_list, (size_t(c->height) + 1) * sizeof(uint32_t)));
  RDL_TRY(rdl::FastCompactRows(c->s, row_mask, c->height, c->rows_list,
                               c->rows_list + c->height));
  c->rows_list_mask = row_mask;
  return RDL_OK;
}

int LaunchRowsForward(rdl_conv* c, const float* in, uint32_t in_w, uint32_t in_h,
                      uint32_t ox, uint32_t oy, void* spec, const uint8_t* row_mask) {
  if (c->tiled) {
    if (row_mask) {
      rdl::SetError("LDS FFT: row masks need the row-major (float64) plans");
      return RDL_ERR_UNSUPPORTED;
    }
    return rdl::FastRowsForwardLaunch(c->s, c->fast_rows, in, spec, c->tw_row, c->ptw_row,
                                      c->height, in_w, in_h, ox, oy, nullptr, nullptr, 1,
                                      c->twd_row);
  }
  if (c->fast_rows) {
    const size_t row_bytes = size_t(c->width / 2 + 1) * (c->f64 ? 16 : 8);
    if (row_mask) {
      RDL_TRY(CompactRowsFor(c, row_mask, false));
      return rdl::FastRowsForwardLaunch(c->s, c->fast_rows, in, spec, c->tw_row,
                                        c->ptw_row, c->height, in_w, in_h, ox, oy,
                                        c->rows_list, c->rows_list + c->height, 0,
                                        c->twd_row);
    }
    // rows outside the window are zero spectra
    char* base = static_cast<char*>(spec);
    if (oy > 0) RDL_HIP_CHECK(hipMemsetAsync(base, 0, size_t(oy) * row_bytes, c->s->stream));
    if (oy + in_h < c->height)
      RDL_HIP_CHECK(hipMemsetAsync(base + size_t(oy + in_h) * row_bytes, 0,
                                   size_t(c->height - oy - in_h) * row_bytes,
                                   c->s->stream));
    return rdl::FastRowsForwardLaunch(c->s, c->fast_rows, in, spec, c->tw_row, c->ptw_row,
                                      c->height, in_w, in_h, ox, oy, nullptr, nullptr, 0,
                                      c->twd_row);
  }
  return rdl::LdsRowsForwardLaunch(c->s, c->row_plan, c->f64, c->row_count, c->height, in,
                                   in_w, in_h, ox, oy, spec, row_mask);
}

int LaunchRowsInverse(rdl_conv* c, const void* spec, float* out, uint32_t out_w,
                      uint32_t out_h, uint32_t ox, uint32_t oy, int subtract) {
  if (c->fast_rows)
    return rdl::FastRowsInverseLaunch(c->s, c->fast_rows, spec, out, c->tw_row, c->ptw_row,
                                      c->height, out_w, out_h, ox, oy, subtract,
                                      c->tiled ? 1 : 0, nullptr, c->twd_row);
  return rdl::LdsRowsInverseLaunch(c->s, c->row_plan, c->f64, c->row_count, c->height, spec,
                                   out, out_w, out_h, ox, oy, subtract);
}

// the column pass of any mode through the split passes (see rdl::LdsSplit)
int LaunchColumnsSplit(rdl_conv* c, const void* in, void* out, const void* kern, int mode,
                       double scale, const uint8_t* row_mask) {
  auto pass = [&](bool b, int m, const void* i, void* o, const void* k, double sc,
                  const uint8_t* mask) {
    return rdl::LdsColumnsSplitLaunch(c->s, c->sp, c->col_plan, c->f64, c->width, b, m, i, o, k,
                                      sc, mask);
  };
  const size_t bytes = size_t(SpectrumBytes(c));
  if (mode == 0) {  // A: in -> scratch, B: scratch -> out (natural order)
    RDL_TRY(EnsureLaneScratch(c, bytes));
    RDL_TRY(pass(false, 0, in, c->scratch, nullptr, 1.0, row_mask));
    return pass(true, 0, c->scratch, out, nullptr, 1.0, nullptr);
  }
  if (mode == 1) {  // A: in -> out, B (fwd x K x s inv) and A^-1 in place
    RDL_TRY(pass(false, 0, in, out, nullptr, 1.0, row_mask));
    RDL_TRY(pass(true, 1, out, out, kern, scale, nullptr));
    return pass(false, 1, out, out, nullptr, 1.0, nullptr);
  }
  // mode 2: B (x K x s inv) from the natural spectrum into scratch, A^-1 -> out
  RDL_TRY(EnsureLaneScratch(c, bytes));
  RDL_TRY(pass(true, 2, in, c->scratch, kern, scale, nullptr));
  return pass(false, 1, c->scratch, out, nullptr, 1.0, nullptr);
}

int LaunchColumns(rdl_conv* c, const void* in, void* out, const void* kern,
                  int mode, double scale, const uint8_t* row_mask, int kern_cm,
                  int out_cm, int in_cm = 0) {
  if (c->split) return LaunchColumnsSplit(c, in, out, kern, mode, scale, row_mask);
  if (c->tiled) {
    // four-step passes through the conv's scratch (tiled spectra; the
    // layout flags do not apply)
    if (row_mask) {
      rdl::SetError("LDS FFT: row masks need the row-major (float64) plans");
      return RDL_ERR_UNSUPPORTED;
    }
    RDL_TRY(EnsureLaneScratch(c, size_t(SpectrumBytes(c))));
    const uint32_t nc = c->width / 2 + 1;
    const float sc = float(scale);
    auto step = [&](bool b, const void* i, void* o, int inv) {
      return rdl::FastStepLaunch(c->s, c->steps, b, i, o, kern, c->tw_col,
                                 b ? c->ptw_b : c->ptw_a, nc, inv, sc);
    };
    if (mode != 2) {
      RDL_TRY(step(false, in, c->scratch, 0));
      RDL_TRY(step(true, c->scratch, out, 0));
      if (mode == 0) return RDL_OK;
      in = out;
    }
    RDL_TRY(step(false, in, c->scratch, 1));
    return step(true, c->scratch, out, 1);
  }
  if (c->fast_cols) {
    const uint32_t* rows = nullptr;
    const uint32_t* n_rows = nullptr;
    if (row_mask && mode != 2) {
      RDL_TRY(CompactRowsFor(c, row_mask, true));
      rows = c->rows_list;
      n_rows = c->rows_list + c->height;
      c->rows_list_mask = nullptr;  // the mask's contents may change next time
    }
    if (c->conv_cols && mode == 1 && !in_cm && (!out_cm || in != out))
      return rdl::ConvColumnsDLaunch(c->s, c->conv_cols, in, out, kern, c->tw_col,
                                     c->width / 2 + 1, kern_cm, out_cm, rows, n_rows, 0,
                                     c->height, scale);
    return rdl::FastColumnsLaunch(c->s, c->fast_cols, in, out, kern, c->ptw_col,
                                  c->width / 2 + 1, uint32_t(mode), in_cm, out_cm, kern_cm,
                                  rows, n_rows, 0, c->height, scale);
  }
  return rdl::LdsColumnsLaunch(c->s, c->col_plan, c->f64, c->col_count, c->width, in, out,
                               kern, mode, scale, row_mask, kern_cm, out_cm);
}

}  // namespace

extern "C" {

int rdl_conv_create(rdl_session* s, uint32_t width, uint32_t height, int f64,
                    rdl_conv** out) {
  return rdl_conv_create_ex(s, width, height, f64, RDL_CONV_COLUMNS_AUTO, out);
}

int rdl_conv_columns_split(const rdl_conv* c) { return c && c->split ? 1 : 0; }

int rdl_conv_create_ex(rdl_session* s, uint32_t width, uint32_t height, int f64,
                       int columns, rdl_conv** out) {
  RDL_ARG_CHECK(s && out, "NULL argument");
  RDL_ARG_CHECK(columns >= RDL_CONV_COLUMNS_AUTO && columns <= RDL_CONV_COLUMNS_SPLIT,
                "bad column strategy");
  RDL_ARG_CHECK(width >= 2 && height >= 2, "bad size");
  *out = nullptr;
  // the planning arithmetic of this function: lds_fft_plan.h
  const size_t max_elems = rdl::LdsMaxLength(f64 != 0);
  if (width > max_elems || height > max_elems) {
    rdl::SetError("LDS FFT: size exceeds LDS capacity");
    return RDL_ERR_UNSUPPORTED;
  }
  auto c = std::make_unique<rdl_conv>();
  c->s = s;
  c->width = width;
  c->height = height;
  c->f64 = f64 != 0;
  RDL_HIP_CHECK(hipSetDevice(s->device));
  RDL_TRY(rdl::MakeLdsPlan(s, width, c->f64, &c->row_plan, &c->tw_row));
  RDL_TRY(rdl::MakeLdsPlan(s, height, c->f64, &c->col_plan, &c->tw_col));
  c->row_count = rdl::LdsTransformsPerWorkgroup(width, c->f64);
  c->col_count = rdl::LdsTransformsPerWorkgroup(height, c->f64);
  // split columns: N = N1 * N2 with N1 the largest divisor <= sqrt(N)
  const rdl::LdsSplitFactors sf = rdl::ChooseLdsSplit(height, c->f64);
  const uint32_t n1 = sf.n1, n2 = sf.n2;
  const bool can_split = sf.can_split;
  // AUTO keeps the single pass: measured on MI355X (tools/bench_fft.py) the
  // split passes are faster only for the shared-spectrum inverse in float
  // (8192^2: 606 vs 909 us) and slower for the fused convolutions
  const bool want_split = columns == RDL_CONV_COLUMNS_SPLIT;
  if (want_split && !can_split) {
    rdl::SetError("LDS FFT: column length " + std::to_string(height) +
                  " has no split into two factors >= 4");
    return RDL_ERR_UNSUPPORTED;
  }
  // compile-time-planned kernels for the sizes that have one
  // (RDL_FFT_FAST=0 keeps the runtime-plan kernels, for comparison)
  const char* fast_env = std::getenv("RDL_FFT_FAST");
  const bool fast_ok = !(fast_env && fast_env[0] == '0') && !want_split;
  if (fast_ok) {
    c->fast_cols = rdl::FindFastColumns(height, c->f64);
    if (c->f64) c->conv_cols = rdl::FindConvColumnsD(height);
    if (width % 2 == 0) c->fast_rows = rdl::FindFastRows(width, c->f64);
    // float planes: four-step column passes where the length has a plan
    if (!c->f64 && c->fast_rows) {
      c->steps = rdl::FindFastSteps(height);
      c->tiled = c->steps != nullptr;
    }
    // the row kernels' pass twiddles: double plans read the global pass
    // table, float plans compute theirs from the two-level base in LDS
    if (c->fast_rows && c->f64)
      RDL_TRY(rdl::MakePassTable(width / 2, c->fast_rows->radix, c->f64, &c->ptw_row, c->s->stream));
    if (c->fast_rows && !c->f64)
      RDL_TRY(rdl::MakeTwiddleBase(width, &c->twd_row, c->s->stream));
    if (c->fast_cols)
      RDL_TRY(rdl::MakePassTable(height, c->fast_cols->radix, c->f64, &c->ptw_col, c->s->stream));
    if (c->steps) {
      RDL_TRY(rdl::MakePassTable(c->steps->n1, c->steps->radix_a, false, &c->ptw_a, c->s->stream));
      RDL_TRY(rdl::MakePassTable(c->steps->n2, c->steps->radix_b, false, &c->ptw_b, c->s->stream));
    }
  }
  if (want_split) {
    c->split = true;
    c->sp.n1 = n1;
    c->sp.n2 = n2;
    RDL_TRY(rdl::MakeLdsPlan(s, n1, c->f64, &c->sp.plan_n1, &c->tw_n1));
    RDL_TRY(rdl::MakeLdsPlan(s, n2, c->f64, &c->sp.plan_n2, &c->tw_n2));
    c->sp.cols = sf.cols;
  }
  // RDL_LOG_FFT_PLANS=1: one line per plan (sizes, precision, which kernels)
  static const bool log_plans = [] {
    const char* e = std::getenv("RDL_LOG_FFT_PLANS");
    return e && e[0] == '1';
  }();
  if (log_plans)
    std::fprintf(stderr, "[fft-plan] %ux%u %s rows=%s cols=%s\n", width, height,
                 c->f64 ? "f64" : "f32", c->fast_rows ? "fast" : "runtime",
                 c->tiled ? "four-step" : c->fast_cols ? "fast" : "runtime");
  *out = c.release();
  return RDL_OK;
}

int rdl_conv_destroy(rdl_conv* c) {
  if (!c) return RDL_OK;
  if (rdl::ShutDown()) return RDL_OK;  // its blocks were released by rdl_shutdown
  (void)hipStreamSynchronize(c->s->stream);
  if (c->tw_row) (void)rdl::DevFree(c->tw_row);
  if (c->tw_col) (void)rdl::DevFree(c->tw_col);
  if (c->tw_n1) (void)rdl::DevFree(c->tw_n1);
  if (c->tw_n2) (void)rdl::DevFree(c->tw_n2);
  for (void* p : c->scratch_lane)
    if (p) (void)rdl::DevFree(p);
  if (c->rows_list) (void)rdl::DevFree(c->rows_list);
  for (void* p : {c->ptw_row, c->ptw_col, c->ptw_a, c->ptw_b, c->twd_row, c->cos_w, c->cos_h,
                  c->real_a.ptr})
    if (p) (void)rdl::DevFree(p);
  delete c;
  return RDL_OK;
}

size_t rdl_conv_spectrum_bytes(const rdl_conv* c) {
  return c ? size_t(SpectrumBytes(c)) : 0;
}

int rdl_conv_rows_forward(rdl_conv* c, const float* d_in, uint32_t in_w,
                          uint32_t in_h, uint32_t ox, uint32_t oy, void* d_spec) {
  RDL_ARG_CHECK(c && d_in && d_spec, "NULL argument");
  RDL_ARG_CHECK(uint64_t(ox) + in_w <= c->width && uint64_t(oy) + in_h <= c->height,
                "input window outside the plane");
  rdl::ScopedTiming t(c->s, c->f64 ? "conv64_rows" : "conv_rows",
                      double(in_w) * in_h * 4.0 + SpectrumBytes(c));
  return LaunchRowsForward(c, d_in, in_w, in_h, ox, oy, d_spec, nullptr);
}

int rdl_conv_rows_forward_masked(rdl_conv* c, const float* d_in, uint32_t in_w,
                                 uint32_t in_h, uint32_t ox, uint32_t oy,
                                 void* d_spec, const uint8_t* d_row_mask) {
  RDL_ARG_CHECK(c && d_in && d_spec && d_row_mask, "NULL argument");
  RDL_ARG_CHECK(uint64_t(ox) + in_w <= c->width && uint64_t(oy) + in_h <= c->height,
                "input window outside the plane");
  // bytes depend on the mask's occupancy (known only on the device): the
  // sparse family reports time and launches, not bandwidth
  rdl::ScopedTiming t(c->s, c->f64 ? "conv64_rows_sparse" : "conv_rows_sparse", 0.0);
  return LaunchRowsForward(c, d_in, in_w, in_h, ox, oy, d_spec, d_row_mask);
}

int rdl_conv_columns(rdl_conv* c, const void* d_in, void* d_out,
                     const void* d_kernel, int mode, double scale) {
  RDL_ARG_CHECK(c && d_in && d_out, "NULL argument");
  RDL_ARG_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
  RDL_ARG_CHECK(mode == 0 || d_kernel, "kernel spectrum required");
  const double sb = SpectrumBytes(c);
  rdl::ScopedTiming t(c->s, c->f64 ? "conv64_cols" : "conv_cols",
                      mode == 0 ? 2.0 * sb : 3.0 * sb);
  return LaunchColumns(c, d_in, d_out, d_kernel, mode, scale, nullptr, 0, 0);
}

int rdl_conv_columns_ex(rdl_conv* c, const void* d_in, void* d_out,
                        const void* d_kernel, int mode, double scale,
                        const uint8_t* d_row_mask, int kernel_layout,
                        int out_layout) {
  RDL_ARG_CHECK(c && d_in && d_out, "NULL argument");
  RDL_ARG_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
  RDL_ARG_CHECK(mode == 0 || d_kernel, "kernel spectrum required");
  RDL_ARG_CHECK(out_layout == RDL_CONV_ROW_MAJOR ||
                    ((mode == 0 || (mode == 1 && c->conv_cols)) && d_out != d_in),
                "a column-major output needs mode 0 (or mode 1 with a float64 "
                "convolution-column plan) and a separate output");
  RDL_ARG_CHECK(kernel_layout == RDL_CONV_ROW_MAJOR ||
                    kernel_layout == RDL_CONV_COL_MAJOR,
                "bad kernel layout");
  RDL_ARG_CHECK(!c->split || (kernel_layout == RDL_CONV_ROW_MAJOR &&
                              out_layout == RDL_CONV_ROW_MAJOR),
                "split column plans use the row-major layout only");
  const double sb = SpectrumBytes(c);
  // with a row mask the input reads are skipped for the zero rows: count
  // the kernel read and the output write only (a lower bound)
  const char* fam = d_row_mask ? (c->f64 ? "conv64_cols_sparse" : "conv_cols_sparse")
                               : (c->f64 ? "conv64_cols" : "conv_cols");
  const double bytes = d_row_mask ? (mode == 0 ? sb : 2.0 * sb)
                                  : (mode == 0 ? 2.0 * sb : 3.0 * sb);
  rdl::ScopedTiming t(c->s, fam, bytes);
  const int kcm = kernel_layout == RDL_CONV_COL_MAJOR;
  const int ocm = out_layout == RDL_CONV_COL_MAJOR;
  return LaunchColumns(c, d_in, d_out, d_kernel, mode, scale, d_row_mask, kcm, ocm);
}

int rdl_conv_columns_window(rdl_conv* c, const void* d_in, void* d_out,
                            const void* d_kernel, double scale, const uint8_t* d_row_mask,
                            int kernel_layout, uint32_t out_row0, uint32_t out_rows,
                            int kernel_f32) {
  RDL_ARG_CHECK(c && d_in && d_out && d_kernel, "NULL argument");
  RDL_ARG_CHECK(uint64_t(out_row0) + out_rows <= c->height, "output rows outside the plane");
  RDL_ARG_CHECK(kernel_layout == RDL_CONV_ROW_MAJOR || kernel_layout == RDL_CONV_COL_MAJOR,
                "bad kernel layout");
  const bool convd = c->f64 && c->conv_cols;
  RDL_ARG_CHECK(!kernel_f32 || convd, "a float kernel needs a float64 convolution-column plan");
  if (!convd)
    return rdl_conv_columns_ex(c, d_in, d_out, d_kernel, 1, scale, d_row_mask, kernel_layout,
                               RDL_CONV_ROW_MAJOR);
  const double sb = SpectrumBytes(c);
  const double win = sb * double(out_rows) / double(c->height);
  const double kb = kernel_f32 ? 0.5 * sb : sb;
  const char* fam = d_row_mask ? "conv64_cols_sparse" : "conv64_cols";
  rdl::ScopedTiming t(c->s, fam, d_row_mask ? kb + win : kb + sb + win);
  const uint32_t* rows = nullptr;
  const uint32_t* n_rows = nullptr;
  if (d_row_mask) {
    RDL_TRY(CompactRowsFor(c, d_row_mask, true));
    rows = c->rows_list;
    n_rows = c->rows_list + c->height;
    c->rows_list_mask = nullptr;  // the mask's contents may change next time
  }
  return rdl::ConvColumnsDLaunch(c->s, c->conv_cols, d_in, d_out, d_kernel, c->tw_col,
                                 c->width / 2 + 1, kernel_layout == RDL_CONV_COL_MAJOR, 0, rows,
                                 n_rows, 0, c->height, scale, out_row0, out_rows,
                                 kernel_f32 != 0);
}

namespace {
// the float64 convolution-column plans keep the correction's spectrum in the
// tiled layout (RDL_CONV64_TILED=0: row-major, for comparison)
bool Tiled64(const rdl_conv* c) {
  static const bool on = [] {
    const char* e = std::getenv("RDL_CONV64_TILED");
    return !(e && e[0] == '0');
  }();
  return on && c->f64 && c->conv_cols && c->fast_rows && !c->tiled;
}
}  // namespace

size_t rdl_conv_convolve_subtract_bytes(const rdl_conv* c) {
  if (!c) return 0;
  return Tiled64(c) ? rdl::TiledComplexCount(c->width, c->height) * 16
                    : size_t(SpectrumBytes(c));
}

namespace {
// rdl_conv_convolve_subtract; `peak` (plans with compile-time rows only): the
// fused search of the inverse row pass, one partial per image row
int ConvolveSubtract(rdl_conv* c, const float* d_image, uint32_t img_w, uint32_t img_h,
                     uint32_t ox, uint32_t oy, const void* d_kernel, int kernel_layout,
                     int kernel_f32, double scale, const uint8_t* d_row_mask, void* d_work,
                     float* d_residual, const rdl::RowPeak* peak) {
  RDL_ARG_CHECK(c && d_image && d_kernel && d_work && d_residual, "NULL argument");
  RDL_ARG_CHECK(uint64_t(ox) + img_w <= c->width && uint64_t(oy) + img_h <= c->height,
                "image window outside the plane");
  if (!Tiled64(c)) {
    RDL_TRY(d_row_mask
                ? rdl_conv_rows_forward_masked(c, d_image, img_w, img_h, ox, oy, d_work,
                                               d_row_mask)
                : rdl_conv_rows_forward(c, d_image, img_w, img_h, ox, oy, d_work));
    // The runtime row kernels transform plane rows 2t and 2t + 1 as one
    // complex row, so the partner of the window's first or last row needs a
    // spectrum as well: the convolution columns write their window only, and
    // with a mask the forward rows leave the rows of an all-zero workgroup
    // as they were. Whatever d_work held there would reach the window's row
    // through the shared transform's rounding.
    uint32_t win0 = oy, win_end = oy + img_h;
    if (!c->fast_rows) {
      win0 &= ~1u;
      win_end = std::min(c->height, (win_end + 1) & ~1u);
    }
    RDL_TRY(rdl_conv_columns_window(c, d_work, d_work, d_kernel, scale, d_row_mask,
                                    kernel_layout, win0, win_end - win0, kernel_f32));
    if (!peak) return rdl_conv_rows_inverse(c, d_work, d_residual, img_w, img_h, ox, oy, 1);
    // rdl_conv_rows_inverse's launch on these plans, with the search
    rdl::ScopedTiming t(c->s, c->f64 ? "conv64_rows" : "conv_rows",
                        SpectrumBytes(c) + double(img_w) * img_h * 8.0);
    return rdl::FastRowsInverseLaunch(c->s, c->fast_rows, d_work, d_residual, c->tw_row,
                                      c->ptw_row, c->height, img_w, img_h, ox, oy, 1,
                                      c->tiled ? 1 : 0, peak, c->twd_row);
  }
  RDL_ARG_CHECK(kernel_layout == RDL_CONV_ROW_MAJOR || kernel_layout == RDL_CONV_COL_MAJOR,
                "bad kernel layout");
  // the same three passes on the tiled layout: the row passes move whole
  // 256-byte tile rows, the column pass reads and writes column c at a
  // 256-byte stride inside its tile (not a full row stride)
  const double sb = SpectrumBytes(c);
  const double win = sb * double(img_h) / double(c->height);
  const uint32_t* rows = nullptr;
  const uint32_t* n_rows = nullptr;
  {
    rdl::ScopedTiming t(c->s, d_row_mask ? "conv64_rows_sparse" : "conv64_rows",
                        d_row_mask ? 0.0 : double(img_w) * img_h * 4.0 + win);
    if (d_row_mask) {
      RDL_TRY(CompactRowsFor(c, d_row_mask, false));
      rows = c->rows_list;
      n_rows = c->rows_list + c->height;
    }
    RDL_TRY(rdl::FastRowsForwardLaunch(c->s, c->fast_rows, d_image, d_work, c->tw_row,
                                       c->ptw_row, c->height, img_w, img_h, ox, oy, rows,
                                       n_rows, 1, c->twd_row, 0));
  }
  {
    const double kb = kernel_f32 ? 0.5 * sb : sb;
    rdl::ScopedTiming t(c->s, d_row_mask ? "conv64_cols_sparse" : "conv64_cols",
                        d_row_mask ? kb + win : kb + 2.0 * win);
    // unmasked: the rows outside the window are zero (never written)
    RDL_TRY(rdl::ConvColumnsDLaunch(c->s, c->conv_cols, d_work, d_work, d_kernel, c->tw_col,
                                    c->width / 2 + 1, kernel_layout == RDL_CONV_COL_MAJOR, 0,
                                    rows, n_rows, oy, img_h, scale, oy, img_h,
                                    kernel_f32 != 0, true));
    c->rows_list_mask = nullptr;  // the mask's contents may change next time
  }
  rdl::ScopedTiming t(c->s, "conv64_rows", win + double(img_w) * img_h * 8.0);
  return rdl::FastRowsInverseLaunch(c->s, c->fast_rows, d_work, d_residual, c->tw_row,
                                    c->ptw_row, c->height, img_w, img_h, ox, oy, 1, 1, peak,
                                    c->twd_row);
}
}  // namespace

int rdl_conv_convolve_subtract(rdl_conv* c, const float* d_image, uint32_t img_w,
                               uint32_t img_h, uint32_t ox, uint32_t oy,
                               const void* d_kernel, int kernel_layout, int kernel_f32,
                               double scale, const uint8_t* d_row_mask, void* d_work,
                               float* d_residual) {
  return ConvolveSubtract(c, d_image, img_w, img_h, ox, oy, d_kernel, kernel_layout,
                          kernel_f32, scale, d_row_mask, d_work, d_residual, nullptr);
}

int rdl_conv_convolve_subtract_peak(rdl_conv* c, const float* d_image, uint32_t img_w,
                                    uint32_t img_h, uint32_t ox, uint32_t oy,
                                    const void* d_kernel, int kernel_layout, int kernel_f32,
                                    double scale, const uint8_t* d_row_mask, void* d_work,
                                    float* d_residual, uint32_t h_border, uint32_t v_border,
                                    int allow_negative, const uint8_t* d_mask,
                                    int avx_semantics, uint32_t slot) {
  RDL_ARG_CHECK(c, "NULL argument");
  RDL_ARG_CHECK(slot < RDL_PEAK_SLOTS, "peak slot out of range");
  RDL_ARG_CHECK(img_w > 0 && img_h > 0, "empty image");
  RDL_ARG_CHECK(uint64_t(img_w) * img_h < 0xffffffffull,
                "image too large for 32-bit pixel index");
  if (!c->fast_rows) {  // the runtime-plan row kernels have no search
    RDL_TRY(ConvolveSubtract(c, d_image, img_w, img_h, ox, oy, d_kernel, kernel_layout,
                             kernel_f32, scale, d_row_mask, d_work, d_residual, nullptr));
    return RDL_NOT_FUSED;
  }
  rdl_session* s = c->s;
  rdl::RowPeak pk{};
  const rdl::PeakBox box = rdl::MakePeakBox(img_w, img_h, h_border, v_border);
  pk.xs = box.xs;
  pk.xe = box.xe;
  pk.ys = box.ys;
  pk.ye = box.ye;
  pk.mask = d_mask;
  pk.allow_negative = allow_negative;
  // the slot's partials area, as rdl_conv_rows_inverse_peak lays them out
  RDL_TRY(s->EnsureScratch(s->partials, RDL_PEAK_SLOTS * size_t(img_h) * sizeof(uint64_t)));
  pk.partials = static_cast<uint64_t*>(s->partials.ptr) + size_t(slot) * img_h;
  RDL_TRY(ConvolveSubtract(c, d_image, img_w, img_h, ox, oy, d_kernel, kernel_layout,
                           kernel_f32, scale, d_row_mask, d_work, d_residual, &pk));
  return rdl::LaunchPeakFinal(s, pk.partials, img_h, d_residual, img_w, img_h, avx_semantics,
                              d_mask != nullptr, rdl::PeakSlot(s, slot));
}

int rdl_conv_columns_layout(rdl_conv* c, const void* d_in, void* d_out,
                            const void* d_kernel, int mode, double scale,
                            const uint8_t* d_row_mask, int in_layout,
                            int kernel_layout, int out_layout) {
  RDL_ARG_CHECK(c && d_in && d_out, "NULL argument");
  RDL_ARG_CHECK(mode >= 0 && mode <= 2, "mode must be 0, 1 or 2");
  RDL_ARG_CHECK(mode == 0 || d_kernel, "kernel spectrum required");
  for (int l : {in_layout, kernel_layout, out_layout})
    RDL_ARG_CHECK(l == RDL_CONV_ROW_MAJOR || l == RDL_CONV_COL_MAJOR, "bad layout");
  RDL_ARG_CHECK(c->tiled || in_layout == RDL_CONV_ROW_MAJOR || mode == 2,
                "a column-major input is a mode-2 spectrum");
  RDL_ARG_CHECK(c->tiled || in_layout == out_layout || d_out != d_in,
                "changing the layout needs a separate output");
  if (!c->fast_cols && !c->tiled) {
    if (in_layout == RDL_CONV_ROW_MAJOR && (out_layout == RDL_CONV_ROW_MAJOR || mode == 0))
      return rdl_conv_columns_ex(c, d_in, d_out, d_kernel, mode, scale, d_row_mask,
                                 kernel_layout, out_layout);
    rdl::SetError("LDS FFT: this layout needs the compile-time-planned column kernels");
    return RDL_ERR_UNSUPPORTED;
  }
  const double sb = SpectrumBytes(c);
  const char* fam = d_row_mask ? (c->f64 ? "conv64_cols_sparse" : "conv_cols_sparse")
                               : (c->f64 ? "conv64_cols" : "conv_cols");
  const double bytes = d_row_mask ? (mode == 0 ? sb : 2.0 * sb)
                                  : (mode == 0 ? 2.0 * sb : 3.0 * sb);
  rdl::ScopedTiming t(c->s, fam, bytes);
  const int icm = in_layout == RDL_CONV_COL_MAJOR;
  const int kcm = kernel_layout == RDL_CONV_COL_MAJOR;
  const int ocm = out_layout == RDL_CONV_COL_MAJOR;
  return LaunchColumns(c, d_in, d_out, d_kernel, mode, scale, d_row_mask, kcm, ocm,
                       icm);
}

int rdl_conv_fast(const rdl_conv* c) {
  if (!c) return 0;
  return (c->fast_cols ? RDL_CONV_FAST_COLUMNS : 0) | (c->fast_rows ? RDL_CONV_FAST_ROWS : 0) |
         (c->tiled ? RDL_CONV_FAST_TILED : 0) |
         (c->f64 && c->conv_cols ? RDL_CONV_FAST_CONVD : 0);
}

int rdl_conv_rows_inverse(rdl_conv* c, const void* d_spec, float* d_out,
                          uint32_t out_w, uint32_t out_h, uint32_t ox, uint32_t oy,
                          int subtract) {
  RDL_ARG_CHECK(c && d_spec && d_out, "NULL argument");
  RDL_ARG_CHECK(uint64_t(ox) + out_w <= c->width && uint64_t(oy) + out_h <= c->height,
                "output window outside the plane");
  rdl::ScopedTiming t(c->s, c->f64 ? "conv64_rows" : "conv_rows",
                      SpectrumBytes(c) + double(out_w) * out_h * (subtract ? 8.0 : 4.0));
  return LaunchRowsInverse(c, d_spec, d_out, out_w, out_h, ox, oy, subtract);
}

int rdl_conv_rows_inverse_peak(rdl_conv* c, const void* d_spec, float* d_out,
                               uint32_t out_w, uint32_t out_h, uint32_t ox, uint32_t oy,
                               uint32_t h_border, uint32_t v_border, int allow_negative,
                               const uint8_t* d_mask, uint32_t slot) {
  RDL_ARG_CHECK(c && d_spec && d_out, "NULL argument");
  RDL_ARG_CHECK(uint64_t(ox) + out_w <= c->width && uint64_t(oy) + out_h <= c->height,
                "output window outside the plane");
  RDL_ARG_CHECK(slot < RDL_PEAK_SLOTS, "peak slot out of range");
  RDL_ARG_CHECK(uint64_t(out_w) * out_h < 0xffffffffull, "image too large for 32-bit index");
  if (!c->fast_rows) {
    rdl::SetError("fused peak search needs the compile-time-planned row kernels");
    return RDL_ERR_UNSUPPORTED;
  }
  rdl_session* s = c->s;
  rdl::RowPeak pk{};
  const rdl::PeakBox box = rdl::MakePeakBox(out_w, out_h, h_border, v_border);
  pk.xs = box.xs;
  pk.xe = box.xe;
  pk.ys = box.ys;
  pk.ye = box.ye;
  pk.mask = d_mask;
  pk.allow_negative = allow_negative;
  // one partials area per peak slot: the scales' searches may run on two
  // session lanes at once
  const size_t rows = std::max<size_t>(out_h, 1);
  RDL_TRY(s->EnsureScratch(s->partials, RDL_PEAK_SLOTS * rows * sizeof(uint64_t)));
  pk.partials = static_cast<uint64_t*>(s->partials.ptr) + slot * rows;
  uint32_t n_partials = 1;
  {
    rdl::ScopedTiming t(s, "conv_rows",
                        SpectrumBytes(c) + double(out_w) * out_h * 4.0);
    if (out_h == 0)
      RDL_HIP_CHECK(hipMemsetAsync(pk.partials, 0, sizeof(uint64_t), s->stream));
    else
      RDL_TRY(rdl::FastRowsInverseLaunch(s, c->fast_rows, d_spec, d_out, c->tw_row,
                                         c->ptw_row, c->height, out_w, out_h, ox, oy, 0,
                                         c->tiled ? 1 : 0, &pk, c->twd_row, &n_partials));
  }
  return rdl::LaunchPeakFinal(s, pk.partials, std::max<uint32_t>(n_partials, 1), d_out, out_w,
                              out_h, 1, d_mask != nullptr, rdl::PeakSlot(s, slot));
}

int rdl_conv_forward(rdl_conv* c, const float* d_in, void* d_spec) {
  RDL_TRY(rdl_conv_rows_forward(c, d_in, c->width, c->height, 0, 0, d_spec));
  return rdl_conv_columns(c, d_spec, d_spec, nullptr, 0, 1.0);
}

size_t rdl_conv_real_kernel_bytes(const rdl_conv* c) {
  return c && c->tiled ? rdl::TiledComplexCount(c->width, c->height) * sizeof(float) : 0;
}

int rdl_conv_real_kernel(rdl_conv* c, const float* h_shape, uint32_t n, void* d_kernel) {
  RDL_ARG_CHECK(c && h_shape && d_kernel, "NULL argument");
  if (!c->tiled) {
    rdl::SetError("rdl_conv_real_kernel: needs a four-step (tiled) float plan");
    return RDL_ERR_UNSUPPORTED;
  }
  RDL_ARG_CHECK(n % 2 == 1 && n <= c->width && n <= c->height,
                "kernel side must be odd and fit the plane");
  for (uint32_t y = 0; y < n; ++y)  // the evaluation assumes the symmetry
    for (uint32_t x = 0; x < n; ++x) {
      const float v = h_shape[x + y * n];
      RDL_ARG_CHECK(v == h_shape[(n - 1 - x) + y * n] && v == h_shape[x + (n - 1 - y) * n],
                    "rdl_conv_real_kernel: the kernel is not symmetric in x and y");
    }
  rdl_session* s = c->s;
  if (!c->cos_w) RDL_TRY(rdl::MakeCosTable(c->width, &c->cos_w, c->s->stream));
  if (!c->cos_h) RDL_TRY(rdl::MakeCosTable(c->height, &c->cos_h, c->s->stream));
  const size_t shape_bytes = size_t(n) * n * sizeof(float);
  RDL_TRY(s->EnsureScratch(s->kernel, shape_bytes));
  RDL_HIP_CHECK(hipMemcpyAsync(s->kernel.ptr, h_shape, shape_bytes, hipMemcpyHostToDevice,
                               s->stream));
  RDL_TRY(s->EnsureScratch(c->real_a, size_t(n / 2 + 1) * (c->width / 2 + 1) * sizeof(double)));
  RDL_TRY(rdl::RealKernelLaunch(s, static_cast<const float*>(s->kernel.ptr), n, c->width,
                                c->height, c->cos_w, c->cos_h, c->real_a.ptr,
                                static_cast<float*>(d_kernel)));
  // the shape scratch is host-written next time: finish with it first
  RDL_HIP_CHECK(hipStreamSynchronize(s->stream));
  return RDL_OK;
}

int rdl_conv_forward_half(rdl_conv* c, const float* d_in, uint32_t in_w, uint32_t in_h,
                          uint32_t ox, uint32_t oy, void* d_half) {
  RDL_ARG_CHECK(c && d_in && d_half, "NULL argument");
  if (!c->tiled) {
    rdl::SetError("rdl_conv_forward_half: needs a four-step (tiled) float plan");
    return RDL_ERR_UNSUPPORTED;
  }
  const double sb = SpectrumBytes(c);
  // rows into the lane's scratch, A from there into d_half (A is not
  // in-place safe: rows n2 + N2 n1 -> k1 N2 + n2)
  RDL_TRY(EnsureLaneScratch(c, size_t(sb)));
  void* rows = c->scratch;
  RDL_TRY(rdl_conv_rows_forward(c, d_in, in_w, in_h, ox, oy, rows));
  // algorithmic bytes (the one-pass minimum of the column work, counted per
  // iteration as 2 sb for the forward columns + 2.5 sb per scale: spectrum
  // read, real kernel read, result write), attributed to the three launches
  // as A 1 sb, B* 1 + 1.5 sb per scale, A* 1 sb; the four-step passes move
  // 2, 1 + 1.5 per scale and 2 (the intermediates): PMC shows the ratio
  rdl::ScopedTiming t(c->s, "conv_cols", sb);
  return rdl::FastStepLaunch(c->s, c->steps, false, rows, d_half, nullptr, c->tw_col, c->ptw_a,
                             c->width / 2 + 1, 0, 1.0f);
}

int rdl_conv_scales(rdl_conv* c, const void* d_half, uint32_t n_scales,
                    const void* const* d_kernels, void* const* d_outs, double scale) {
  RDL_ARG_CHECK(c && d_half && (n_scales == 0 || (d_kernels && d_outs)), "NULL argument");
  if (!c->tiled) {
    rdl::SetError("rdl_conv_scales: needs a four-step (tiled) float plan");
    return RDL_ERR_UNSUPPORTED;
  }
  for (uint32_t i = 0; i < n_scales; ++i)
    RDL_ARG_CHECK(d_kernels[i] && d_outs[i] && d_outs[i] != d_half, "bad kernel / output");
  const double sb = SpectrumBytes(c);
  // algorithmic (see rdl_conv_forward_half): the forward columns' write, and
  // per scale the spectrum and real-kernel reads
  rdl::ScopedTiming t(c->s, "conv_cols", sb + n_scales * 1.5 * sb);
  return rdl::FastScalesLaunch(c->s, c->steps, d_half, c->tw_col, c->ptw_b, c->width / 2 + 1,
                               n_scales, reinterpret_cast<const float* const*>(d_kernels),
                               d_outs, float(scale));
}

int rdl_conv_scale_finish(rdl_conv* c, const void* d_in, void* d_out) {
  RDL_ARG_CHECK(c && d_in && d_out && d_in != d_out, "NULL or aliased argument");
  if (!c->tiled) {
    rdl::SetError("rdl_conv_scale_finish: needs a four-step (tiled) float plan");
    return RDL_ERR_UNSUPPORTED;
  }
  // algorithmic (see rdl_conv_forward_half): the scale's result write
  rdl::ScopedTiming t(c->s, "conv_cols", SpectrumBytes(c));
  return rdl::FastStepAInvLaunch(c->s, c->steps, d_in, d_out, c->ptw_a, c->width / 2 + 1);
}

}  // extern "C"
