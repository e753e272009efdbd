// The float64 row plans (the padded residual corrections): 71 plans, two
// kernels each, in a unit of their own so that no FFT unit bounds the build.
// The kernels are fft_fast_rows.h's; the float plans and the launchers are
// in fft_fast_rows.hip.
#include "fft_fast_rows.h"

namespace rdl {

// a double plan's kernels read the global pass tables (no LT, no LDS-DMA)
#define RDL_FAST_ROWS(T, TH, ...)                                                      \
  FastRows {                                                                           \
    2 * ff::Product<__VA_ARGS__>(), true, TH,                                          \
        reinterpret_cast<const void*>(&ff::RowsInverse<T, TH, false, __VA_ARGS__>),    \
        reinterpret_cast<const void*>(&ff::RowsForward<T, TH, false, __VA_ARGS__>),    \
        MakeRadixList<__VA_ARGS__>(), nullptr, 0, nullptr, 0                           \
  }

const FastRows* FindFastRowsD(uint32_t n) {
  static const FastRows kPlans[] = {
      RDL_FAST_ROWS(double, 512, 7, 9, 9, 8),      // 9072
      RDL_FAST_ROWS(double, 512, 9, 8, 8, 8),      // 9216
      RDL_FAST_ROWS(double, 512, 7, 3, 7, 8, 4),   // 9408
      RDL_FAST_ROWS(double, 512, 7, 5, 3, 5, 9),   // 9450
      RDL_FAST_ROWS(double, 256, 7, 9, 9, 4),      // 4536
      RDL_FAST_ROWS(double, 256, 9, 4, 4, 4, 4),   // 4608
      RDL_FAST_ROWS(double, 256, 7, 3, 7, 4, 4),   // 4704
      RDL_FAST_ROWS(double, 256, 5, 3, 5, 8, 4),   // 4800
      RDL_FAST_ROWS(double, 256, 5, 5, 5, 5, 4),   // 5000
      RDL_FAST_ROWS(double, 128, 7, 5, 5, 3),            // 1050
      RDL_FAST_ROWS(double, 128, 5, 9, 3, 4),            // 1080
      RDL_FAST_ROWS(double, 128, 7, 5, 4, 4),            // 1120
      RDL_FAST_ROWS(double, 128, 7, 9, 9),               // 1134
      RDL_FAST_ROWS(double, 128, 9, 8, 8),               // 1152
      RDL_FAST_ROWS(double, 128, 7, 7, 3, 4),            // 1176
      RDL_FAST_ROWS(double, 128, 5, 5, 3, 8),            // 1200
      RDL_FAST_ROWS(double, 128, 5, 5, 5, 5),            // 1250
      RDL_FAST_ROWS(double, 128, 7, 5, 9, 2),            // 1260
      RDL_FAST_ROWS(double, 128, 5, 8, 4, 4),            // 1280
      RDL_FAST_ROWS(double, 128, 9, 9, 8),               // 1296
      RDL_FAST_ROWS(double, 128, 7, 3, 8, 4),            // 1344
      RDL_FAST_ROWS(double, 128, 7, 7, 7, 2),            // 1372
      RDL_FAST_ROWS(double, 128, 7, 5, 5, 4),            // 1400
      RDL_FAST_ROWS(double, 128, 5, 9, 4, 4),            // 1440
      RDL_FAST_ROWS(double, 128, 9, 9, 9),               // 1458
      RDL_FAST_ROWS(double, 128, 7, 7, 5, 3),            // 1470
      RDL_FAST_ROWS(double, 128, 5, 5, 5, 3, 2),         // 1500
      RDL_FAST_ROWS(double, 128, 7, 9, 3, 4),            // 1512
      RDL_FAST_ROWS(double, 128, 3, 8, 8, 4),            // 1536
      RDL_FAST_ROWS(double, 128, 7, 7, 4, 4),            // 1568
      RDL_FAST_ROWS(double, 128, 5, 9, 9, 2),            // 1620
      RDL_FAST_ROWS(double, 128, 7, 5, 3, 8),            // 1680
      RDL_FAST_ROWS(double, 128, 7, 5, 9, 3),            // 1890
      RDL_FAST_ROWS(double, 256, 5, 3, 8, 8),         // 1920
      RDL_FAST_ROWS(double, 256, 9, 9, 3, 4),         // 1944
      RDL_FAST_ROWS(double, 256, 7, 7, 5, 4),         // 1960
      RDL_FAST_ROWS(double, 256, 5, 5, 5, 8),         // 2000
      RDL_FAST_ROWS(double, 256, 7, 9, 8, 2),         // 2016
      RDL_FAST_ROWS(double, 256, 8, 8, 8, 2),         // 2048
      RDL_FAST_ROWS(double, 256, 7, 5, 5, 3, 2),      // 2100
      RDL_FAST_ROWS(double, 256, 5, 9, 3, 8),         // 2160
      RDL_FAST_ROWS(double, 256, 7, 5, 8, 4),         // 2240
      RDL_FAST_ROWS(double, 256, 5, 5, 5, 9),         // 2250
      RDL_FAST_ROWS(double, 256, 7, 9, 9, 2),         // 2268
      RDL_FAST_ROWS(double, 256, 9, 8, 8, 2),         // 2304
      RDL_FAST_ROWS(double, 256, 7, 7, 3, 8),         // 2352
      RDL_FAST_ROWS(double, 256, 5, 5, 3, 8, 2),      // 2400
      RDL_FAST_ROWS(double, 256, 5, 9, 9, 3),         // 2430
      RDL_FAST_ROWS(double, 256, 7, 7, 5, 5),         // 2450
      RDL_FAST_ROWS(double, 256, 5, 5, 5, 5, 2),      // 2500
      RDL_FAST_ROWS(double, 256, 7, 5, 9, 4),         // 2520
      RDL_FAST_ROWS(double, 256, 5, 8, 8, 4),         // 2560
      RDL_FAST_ROWS(double, 256, 9, 9, 8, 2),         // 2592
      RDL_FAST_ROWS(double, 256, 7, 7, 9, 3),         // 2646
      RDL_FAST_ROWS(double, 256, 7, 3, 8, 8),         // 2688
      RDL_FAST_ROWS(double, 256, 7, 7, 7, 4),         // 2744
      RDL_FAST_ROWS(double, 256, 7, 5, 5, 8),         // 2800
      RDL_FAST_ROWS(double, 256, 5, 9, 8, 4),         // 2880
      RDL_FAST_ROWS(double, 256, 9, 9, 9, 2),         // 2916
      RDL_FAST_ROWS(double, 256, 7, 7, 5, 3, 2),      // 2940
      RDL_FAST_ROWS(double, 256, 5, 5, 5, 3, 4),      // 3000
      RDL_FAST_ROWS(double, 256, 7, 9, 3, 8),         // 3024
      RDL_FAST_ROWS(double, 256, 3, 8, 8, 8),         // 3072
      RDL_FAST_ROWS(double, 256, 7, 7, 8, 4),         // 3136
      RDL_FAST_ROWS(double, 256, 7, 5, 5, 9),         // 3150
      RDL_FAST_ROWS(double, 256, 5, 5, 8, 8),         // 3200
      RDL_FAST_ROWS(double, 256, 5, 9, 9, 4),         // 3240
      RDL_FAST_ROWS(double, 256, 7, 5, 3, 8, 2),      // 3360
      RDL_FAST_ROWS(double, 256, 7, 9, 9, 3),         // 3402
      RDL_FAST_ROWS(double, 256, 7, 7, 7, 5),         // 3430
      RDL_FAST_ROWS(double, 256, 7, 5, 5, 5, 2),      // 3500
  };
  for (const FastRows& p : kPlans)
    if (p.n == n) return &p;
  return nullptr;
}

#undef RDL_FAST_ROWS

}  // namespace rdl
