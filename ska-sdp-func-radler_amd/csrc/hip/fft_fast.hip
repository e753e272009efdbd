// Compile-time-planned FFT kernels for the hot transform sizes of the
// multiscale path: the float64 padded residual correction
// (SubMinorLoop::CorrectResidualDirty, cpp/algorithms/subminor_loop.cc:
// 195-218, sizes utils::GetConvolutionSize(scale, W, 1.1)) and the float32
// scale convolutions (MultiScaleTransforms::Transform,
// cpp/algorithms/multiscale/multiscale_transforms.cc:9-21, size W x H).
// Same data layouts and results (to rounding) as lds_fft.hip's runtime-plan
// kernels, which remain the path for every other size.
//
// Why a second engine: the runtime-plan kernels park their waves ~65 % of
// the time (rocprofv3 SQ_WAIT_ANY on MI355X): one 145 KiB double column or
// row pair per CU, the global loads staged through LDS behind a full
// __syncthreads(), generic index arithmetic and out-of-line passes. Here
//   * every pass is specialised at compile time (radix, span, butterflies per
//     thread), fully inlined, twiddles issued before the LDS reads,
//   * workgroups are persistent (one per CU slot) and keep their global
//     traffic in flight across LDS-only barriers: the kernel spectrum column
//     is loaded into registers while the forward column transform runs, the
//     next row pair's spectrum while the current one is transformed,
//   * rows outside the output window are never transformed, sparse inputs
//     (the sub-minor model's occupied rows) are read from a compacted list.
//
// The kernels live one family per unit (fft_fast_cols.hip, fft_fast_convd.hip,
// fft_fast_rows.hip, fft_fast_steps.hip; shared helpers in
// fft_fast_internal.h). Here: what they share on the host (the occupancy
// query, the twiddle and pass tables) and the row-list compaction.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "fft_fast_internal.h"

namespace rdl {
namespace ff {

// row mask (one byte per plane row) -> ascending list of the non-zero rows
__global__ __launch_bounds__(1024) void CompactRows(const uint8_t* __restrict__ mask,
                                                    uint32_t n, uint32_t* __restrict__ rows,
                                                    uint32_t* __restrict__ count) {
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t base;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (tid == 0) base = 0;
  __syncthreads();
  for (uint32_t off = 0; off < n; off += 1024) {
    const uint32_t y = off + tid;
    const bool f = y < n && mask[y] != 0;
    const uint64_t bal = __ballot(f);
    const uint32_t before = __popcll(bal & ((uint64_t(1) << lane) - 1));
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    uint32_t wbase = base;
    for (uint32_t w = 0; w < wave; ++w) wbase += wsum[w];
    if (f) rows[wbase + before] = y;
    __syncthreads();
    if (tid == 0)
      for (uint32_t w = 0; w < 16; ++w) base += wsum[w];
    __syncthreads();
  }
  if (tid == 0) *count = base;
}

}  // namespace ff

// workgroups per CU for a kernel at its LDS size (cached), after raising its
// dynamic LDS limit once per device
int SlotsPerCu(rdl_session* s, const void* fn, uint32_t threads, size_t lds) {
  static std::mutex mutex;
  static std::map<std::tuple<const void*, int, size_t>, int> cache;
  std::lock_guard<std::mutex> lock(mutex);
  const auto key = std::make_tuple(fn, s->device, lds);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  // (below the CU's LDS by the kernel's static arrays: the row kernels'
  // reduction array for the fused peak search and the float rows' twiddle
  // tables)
  hipFuncAttributes attr{};
  if (hipFuncGetAttributes(&attr, fn) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  if (attr.sharedSizeBytes >= kFftLdsBytesFast ||
      hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                          int(kFftLdsBytesFast - attr.sharedSizeBytes)) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, int(threads), lds) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  cache[key] = std::max(n, 1);
  return cache[key];
}

int MakeTwiddleBase(uint32_t base, void** out, hipStream_t stream) {
  // W_base^{64 i} for i < base / 64, then W_base^i for i < 64, in double
  std::vector<double> host;
  auto put = [&](uint64_t e) {
    const long double ang = -2.0L * 3.14159265358979323846264338327950288L *
                            (long double)(e % base) / base;
    host.push_back(double(std::cos(ang)));
    host.push_back(double(std::sin(ang)));
  };
  for (uint32_t i = 0; i < base / ff::kTwdLo; ++i) put(uint64_t(i) * ff::kTwdLo);
  for (uint32_t i = 0; i < ff::kTwdLo; ++i) put(i);
  RDL_HIP_CHECK(rdl::DevMalloc(out, host.size() * sizeof(double)));
  RDL_HIP_CHECK(UploadSync(*out, host.data(), host.size() * sizeof(double), stream));
  return RDL_OK;
}

int MakeCosTable(uint32_t n, void** out, hipStream_t stream) {
  std::vector<double> host(n);
  for (uint32_t j = 0; j < n; ++j)
    host[j] = double(std::cos(2.0L * 3.14159265358979323846264338327950288L *
                              (long double)j / n));
  RDL_HIP_CHECK(rdl::DevMalloc(out, host.size() * sizeof(double)));
  RDL_HIP_CHECK(UploadSync(*out, host.data(), host.size() * sizeof(double), stream));
  return RDL_OK;
}

int MakePassTable(uint32_t n, const RadixList& radix, bool f64, void** out,
                  hipStream_t stream) {
  std::vector<double> re, im;
  uint32_t ns = 1;
  for (uint32_t p = 0; p < radix.n; ++p) {
    const uint32_t r = radix.r[p];
    const uint32_t m = n / (ns * r);
    if (ns > 1)
      for (uint32_t q = 0; q + 1 < r; ++q)
        for (uint32_t k = 0; k < ns; ++k) {
          const uint64_t e = (uint64_t(k) * (q + 1) * m) % n;
          const long double ang =
              -2.0L * 3.14159265358979323846264338327950288L * (long double)e / n;
          re.push_back(double(std::cos(ang)));
          im.push_back(double(std::sin(ang)));
        }
    ns *= r;
  }
  const size_t count = std::max<size_t>(re.size(), 1);
  std::vector<unsigned char> host(count * (f64 ? 16 : 8), 0);
  for (size_t i = 0; i < re.size(); ++i) {
    if (f64) {
      const double v[2] = {re[i], im[i]};
      std::memcpy(&host[i * 16], v, 16);
    } else {
      const float v[2] = {float(re[i]), float(im[i])};
      std::memcpy(&host[i * 8], v, 8);
    }
  }
  RDL_HIP_CHECK(rdl::DevMalloc(out, host.size()));
  RDL_HIP_CHECK(UploadSync(*out, host.data(), host.size(), stream));
  return RDL_OK;
}

int FastCompactRows(rdl_session* s, const uint8_t* mask, uint32_t n, uint32_t* rows,
                    uint32_t* count) {
  ff::CompactRows<<<1, 1024, 0, s->stream>>>(mask, n, rows, count);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

}  // namespace rdl
