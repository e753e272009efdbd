// A whole source catalogue drawn into frequency planes in one call
// (rdl_draw_sources, rdl_hip.h): points and sub-pixel elliptical Gaussians,
// what WSClean's -draw-model and -restore-list need. rdl_draw_gaussian
// (asp.hip) costs a launch per Gaussian; a catalogue has 10^5 to 10^6 rows.
//
// A gather without atomics. Destinations are pixels and contributions are
// computed, not stored, so the image is cut into tiles of 64 x 16 pixels and
// one 256-thread workgroup owns a tile and a chunk of up to 4 planes: every
// pixel has one writer, and its sum runs over the sources in ascending index
// in double, whatever the launch geometry. The host bins the sources' boxes
// into the tiles (a CSR list per tile, indices ascending), and only tiles with
// a list are launched. A workgroup stages its list through LDS 256 sources at
// a time (a coalesced read of the indices, then the records); every thread
// walks the staged chunk in order and tests the source's box against its 4
// row-contiguous pixels: a miss costs compares, a hit one exp per pixel, used
// for every plane of the chunk.
//
// Bound: the exp in double (about 40 double operations) per pixel of a
// Gaussian's box; the planes are read and written once. The weakness is skew:
// a tile under a crowded field runs as long as its list
// (profiles/draw_sources_timing.txt).
#include <algorithm>
#include <chrono>
#include <cmath>

#include "rdl_internal.h"

namespace rdl {
namespace {

constexpr uint32_t kTileW = 64, kTileH = 16;
constexpr uint32_t kDrawThreads = 256;
constexpr uint32_t kPixelsPerThread = 4;
constexpr uint32_t kPlaneChunk = 4;
constexpr uint32_t kStage = 256;  // sources per LDS chunk, one per thread
static_assert(kTileW * kTileH == kDrawThreads * kPixelsPerThread, "a tile is a workgroup's pixels");
static_assert(kStage == kDrawThreads, "a thread stages one source");

struct DrawSourcesArgs {
  const rdl_source_shape* shapes;
  const float* amplitudes;  // n_planes rows of n_sources
  uint32_t n_sources;
  const uint32_t* tiles;    // the tiles that have a list
  const uint32_t* offsets;  // n_tiles + 1 offsets into `list`, by tile number
  const uint32_t* list;
  uint32_t tiles_x;
  uint32_t width, height;
  float* planes;
  size_t plane_stride;
  uint32_t first_plane;  // blockIdx.y's chunk starts at first_plane + NP * blockIdx.y
};

// the pixels a source touches, clipped to the plane: lo > hi when none
__device__ __forceinline__ void ClippedRange(double centre, uint32_t half, uint32_t size, int& lo,
                                             int& hi) {
  const double c = floor(centre + 0.5);
  const double a = fmax(c - double(half), 0.0), b = fmin(c + double(half), double(size) - 1.0);
  if (a > b) {
    lo = 1;
    hi = 0;
  } else {
    lo = int(a);
    hi = int(b);
  }
}

template <int NP>
__global__ __launch_bounds__(kDrawThreads) void DrawSourcesKernel(DrawSourcesArgs p) {
  __shared__ double s_x0[kStage], s_y0[kStage], s_qa[kStage], s_qb[kStage], s_qc[kStage];
  __shared__ int s_xlo[kStage], s_xhi[kStage], s_ylo[kStage], s_yhi[kStage];
  __shared__ float s_amp[NP][kStage];

  const uint32_t tile = p.tiles[blockIdx.x];
  const uint32_t begin = p.offsets[tile], end = p.offsets[tile + 1];
  const uint32_t plane0 = p.first_plane + uint32_t(NP) * blockIdx.y;
  const int y = int((tile / p.tiles_x) * kTileH + threadIdx.x / (kTileW / kPixelsPerThread));
  const int x = int((tile % p.tiles_x) * kTileW +
                    (threadIdx.x % (kTileW / kPixelsPerThread)) * kPixelsPerThread);

  double acc[NP][kPixelsPerThread];
#pragma unroll
  for (int g = 0; g < NP; ++g)
#pragma unroll
    for (int k = 0; k < int(kPixelsPerThread); ++k) acc[g][k] = 0.0;
  uint32_t touched = 0;

  for (uint32_t base = begin; base < end; base += kStage) {
    const uint32_t n = min(kStage, end - base);
    __syncthreads();  // the previous chunk has been walked
    if (threadIdx.x < n) {
      const uint32_t i = p.list[base + threadIdx.x];
      const rdl_source_shape e = p.shapes[i];
      s_x0[threadIdx.x] = e.x0;
      s_y0[threadIdx.x] = e.y0;
      s_qa[threadIdx.x] = e.qa;
      s_qb[threadIdx.x] = e.qb;
      s_qc[threadIdx.x] = e.qc;
      int lo, hi;
      ClippedRange(e.x0, e.half_w, p.width, lo, hi);
      s_xlo[threadIdx.x] = lo;
      s_xhi[threadIdx.x] = hi;
      ClippedRange(e.y0, e.half_h, p.height, lo, hi);
      s_ylo[threadIdx.x] = lo;
      s_yhi[threadIdx.x] = hi;
#pragma unroll
      for (int g = 0; g < NP; ++g)
        s_amp[g][threadIdx.x] = p.amplitudes[size_t(plane0 + g) * p.n_sources + i];
    }
    __syncthreads();
    for (uint32_t j = 0; j < n; ++j) {
      if (y < s_ylo[j] || y > s_yhi[j]) continue;
      const int xlo = s_xlo[j], xhi = s_xhi[j];
      if (x + int(kPixelsPerThread) - 1 < xlo || x > xhi) continue;
      const double dy = double(y) - s_y0[j];
      const double qa = s_qa[j], qb = s_qb[j], qc = s_qc[j], x0 = s_x0[j];
      double amp[NP];
#pragma unroll
      for (int g = 0; g < NP; ++g) amp[g] = double(s_amp[g][j]);
#pragma unroll
      for (int k = 0; k < int(kPixelsPerThread); ++k) {
        if (x + k < xlo || x + k > xhi) continue;
        const double dx = double(x + k) - x0;
        const double value = exp(-0.5 * (qa * dx * dx + 2.0 * qb * dx * dy + qc * dy * dy));
#pragma unroll
        for (int g = 0; g < NP; ++g) acc[g][k] += amp[g] * value;
        touched |= 1u << k;
      }
    }
  }
  if (touched == 0) return;
  // a touched pixel lies inside the plane: the boxes were clipped to it
  const size_t pixel = size_t(y) * p.width + size_t(x);
#pragma unroll
  for (int g = 0; g < NP; ++g) {
    float* dest = p.planes + size_t(plane0 + g) * p.plane_stride + pixel;
    if (touched == 0xfu && (reinterpret_cast<uintptr_t>(dest) & 15u) == 0) {
      float4 v = *reinterpret_cast<float4*>(dest);
      v.x += float(acc[g][0]);
      v.y += float(acc[g][1]);
      v.z += float(acc[g][2]);
      v.w += float(acc[g][3]);
      *reinterpret_cast<float4*>(dest) = v;
    } else {
#pragma unroll
      for (int k = 0; k < int(kPixelsPerThread); ++k)
        if (touched & (1u << k)) dest[k] += float(acc[g][k]);
    }
  }
}

template <int NP>
void LaunchDrawSources(rdl_session* s, const DrawSourcesArgs& a, uint32_t n_tiles,
                       uint32_t n_chunks) {
  DrawSourcesKernel<NP><<<dim3(n_tiles, n_chunks), kDrawThreads, 0, s->stream>>>(a);
}

// the tiles [lo, hi] along one axis that a source's clipped range meets
bool TileRange(double centre, uint32_t half, uint32_t size, uint32_t tile, uint32_t& lo,
               uint32_t& hi) {
  const double c = std::floor(centre + 0.5);
  const double a = std::max(c - double(half), 0.0), b = std::min(c + double(half), double(size) - 1.0);
  if (a > b) return false;
  lo = uint32_t(a) / tile;
  hi = uint32_t(b) / tile;
  return true;
}

}  // namespace
}  // namespace rdl

extern "C" int rdl_draw_sources(rdl_session* s, uint32_t n_sources,
                                const rdl_source_shape* h_shapes, const float* h_amplitudes,
                                uint32_t n_planes, uint32_t width, uint32_t height,
                                float* d_planes, size_t plane_stride) {
  using namespace rdl;
  RDL_ARG_CHECK(s && d_planes, "NULL argument");
  RDL_ARG_CHECK(n_planes >= 1 && n_planes <= RDL_MAX_IMAGES,
                "draw sources: plane count out of range");
  RDL_ARG_CHECK(width >= 1 && height >= 1 && width <= (1u << 30) && height <= (1u << 30),
                "draw sources: bad plane size");
  RDL_ARG_CHECK(plane_stride >= size_t(width) * height, "draw sources: planes overlap");
  if (n_sources == 0) return RDL_OK;
  RDL_ARG_CHECK(h_shapes && h_amplitudes, "NULL argument");
  for (uint32_t i = 0; i != n_sources; ++i) {
    const rdl_source_shape& e = h_shapes[i];
    RDL_ARG_CHECK(std::isfinite(e.x0) && std::isfinite(e.y0) && std::isfinite(e.qa) &&
                      std::isfinite(e.qb) && std::isfinite(e.qc),
                  "draw sources: non-finite shape");
  }

  // ---- the sources' boxes binned into tiles: counts, offsets, then the lists,
  // both passes in ascending source index
  const auto bin_start = std::chrono::steady_clock::now();
  const uint32_t tiles_x = (width + kTileW - 1) / kTileW, tiles_y = (height + kTileH - 1) / kTileH;
  const size_t n_tiles = size_t(tiles_x) * tiles_y;
  RDL_ARG_CHECK(n_tiles < 0x7fffffffu, "draw sources: bad plane size");
  std::vector<uint64_t> counts(n_tiles + 1, 0);
  for (uint32_t i = 0; i != n_sources; ++i) {
    const rdl_source_shape& e = h_shapes[i];
    uint32_t tx0, tx1, ty0, ty1;
    if (!TileRange(e.x0, e.half_w, width, kTileW, tx0, tx1) ||
        !TileRange(e.y0, e.half_h, height, kTileH, ty0, ty1))
      continue;
    for (uint32_t ty = ty0; ty <= ty1; ++ty)
      for (uint32_t tx = tx0; tx <= tx1; ++tx) ++counts[size_t(ty) * tiles_x + tx + 1];
  }
  for (size_t t = 0; t != n_tiles; ++t) counts[t + 1] += counts[t];
  const uint64_t n_entries = counts[n_tiles];
  if (n_entries == 0) return RDL_OK;  // every box misses the plane
  RDL_ARG_CHECK(n_entries <= 0xffffffffull, "draw sources: the tile lists exceed 2^32 entries");
  // one block: [tiles with a list | offsets | lists]
  std::vector<uint32_t> packed;
  for (size_t t = 0; t != n_tiles; ++t)
    if (counts[t + 1] != counts[t]) packed.push_back(uint32_t(t));
  const size_t n_active = packed.size();
  const size_t offsets_at = n_active, list_at = offsets_at + n_tiles + 1;
  packed.resize(list_at + n_entries);
  for (size_t t = 0; t <= n_tiles; ++t) packed[offsets_at + t] = uint32_t(counts[t]);
  std::vector<uint32_t> fill(n_tiles);
  for (size_t t = 0; t != n_tiles; ++t) fill[t] = uint32_t(counts[t]);
  for (uint32_t i = 0; i != n_sources; ++i) {
    const rdl_source_shape& e = h_shapes[i];
    uint32_t tx0, tx1, ty0, ty1;
    if (!TileRange(e.x0, e.half_w, width, kTileW, tx0, tx1) ||
        !TileRange(e.y0, e.half_h, height, kTileH, ty0, ty1))
      continue;
    for (uint32_t ty = ty0; ty <= ty1; ++ty)
      for (uint32_t tx = tx0; tx <= tx1; ++tx)
        packed[list_at + fill[size_t(ty) * tiles_x + tx]++] = i;
  }
  if (TimingOn(s) && FamilyOn("draw_sources_bin")) {
    const std::chrono::duration<double, std::milli> ms =
        std::chrono::steady_clock::now() - bin_start;
    const std::lock_guard<std::recursive_mutex> lock(s->timing_mutex);
    TimingEntry& entry = s->timings["draw_sources_bin"];
    entry.ms += ms.count();
    ++entry.launches;
  }

  // ---- one device block: shapes (8-byte aligned first), amplitudes, lists
  const size_t shape_bytes = size_t(n_sources) * sizeof(rdl_source_shape);
  const size_t amp_bytes = size_t(n_planes) * n_sources * sizeof(float);
  const size_t packed_bytes = packed.size() * sizeof(uint32_t);
  void* block = nullptr;
  RDL_TRY(rdl_malloc(s, shape_bytes + amp_bytes + packed_bytes, &block));
  char* d = static_cast<char*>(block);
  auto upload = [&]() -> int {
    ScopedTiming t(s, "draw_sources_upload", double(shape_bytes + amp_bytes + packed_bytes));
    RDL_HIP_CHECK(hipMemcpyAsync(d, h_shapes, shape_bytes, hipMemcpyHostToDevice, s->stream));
    RDL_HIP_CHECK(hipMemcpyAsync(d + shape_bytes, h_amplitudes, amp_bytes, hipMemcpyHostToDevice,
                                 s->stream));
    RDL_HIP_CHECK(hipMemcpyAsync(d + shape_bytes + amp_bytes, packed.data(), packed_bytes,
                                 hipMemcpyHostToDevice, s->stream));
    return RDL_OK;
  };
  int rc = upload();
  if (rc == RDL_OK) {
    DrawSourcesArgs a;
    a.shapes = reinterpret_cast<const rdl_source_shape*>(d);
    a.amplitudes = reinterpret_cast<const float*>(d + shape_bytes);
    a.n_sources = n_sources;
    const uint32_t* d_packed = reinterpret_cast<const uint32_t*>(d + shape_bytes + amp_bytes);
    a.tiles = d_packed;
    a.offsets = d_packed + offsets_at;
    a.list = d_packed + list_at;
    a.tiles_x = tiles_x;
    a.width = width;
    a.height = height;
    a.planes = d_planes;
    a.plane_stride = plane_stride;
    ScopedTiming t(s, "draw_sources",
                   8.0 * double(n_planes) * double(n_active) * double(kTileW * kTileH));
    const uint32_t full = n_planes / kPlaneChunk, rest = n_planes % kPlaneChunk;
    a.first_plane = 0;
    if (full) LaunchDrawSources<kPlaneChunk>(s, a, uint32_t(n_active), full);
    a.first_plane = full * kPlaneChunk;
    if (rest == 1) LaunchDrawSources<1>(s, a, uint32_t(n_active), 1);
    if (rest == 2) LaunchDrawSources<2>(s, a, uint32_t(n_active), 1);
    if (rest == 3) LaunchDrawSources<3>(s, a, uint32_t(n_active), 1);
    if (hipGetLastError() != hipSuccess) {
      SetError("draw sources: launch failed");
      rc = RDL_ERR_HIP;
    }
  }
  // the copies from `packed` (pageable) must have left it before it goes
  if (hipStreamSynchronize(s->stream) != hipSuccess && rc == RDL_OK) {
    SetError("draw sources: hipStreamSynchronize failed");
    rc = RDL_ERR_HIP;
  }
  const int freed = rdl_free(s, block);
  return rc != RDL_OK ? rc : freed;
}
