// What is done with a finished sub-minor loop's model values: scattered into
// a model plane (GetFullIndividualModel, subminor_loop.cc:186-193), stamped
// with a scale's shape kernel, marked in the auto-mask, or copied to the host.
#include "subminor_internal.h"

namespace rdl {

template <typename T>
__global__ __launch_bounds__(256) void ScatterModel(const uint32_t* pos,
                                                    const float* m,
                                                    uint64_t n_sel,
                                                    T* dest, uint32_t dw,
                                                    uint32_t ox, uint32_t oy,
                                                    int add) {
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < n_sel;
       i += uint64_t(gridDim.x) * blockDim.x) {
    const uint32_t pk = pos[i];
    const size_t d = size_t((pk >> 16) + oy) * dw + (pk & 0xffffu) + ox;
    if (add)
      dest[d] += T(m[i]);
    else
      dest[d] = T(m[i]);
  }
}

// rows of the (untrimmed) model plane that hold a non-zero component
// SubMinorLoop::UpdateAutoMask (subminor_loop.cc:220-228)
__global__ __launch_bounds__(256) void UpdateMaskKernel(const uint32_t* pos,
                                                        const float* m, uint64_t n_sel,
                                                        uint32_t n_img, uint32_t width,
                                                        uint8_t* mask) {
  const uint64_t p = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (p >= n_sel) return;
  bool any = false;
  for (uint32_t k = 0; k < n_img; ++k) any |= m[size_t(k) * n_sel + p] != 0.0f;
  if (any) mask[size_t(pos[p] >> 16) * width + (pos[p] & 0xffffu)] = 1;
}

__global__ __launch_bounds__(256) void MarkModelRows(const uint32_t* pos,
                                                     const float* m, uint64_t n_sel,
                                                     uint8_t* rows, uint32_t oy) {
  for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < n_sel;
       i += uint64_t(gridDim.x) * blockDim.x)
    if (m[i] != 0.0f) rows[(pos[i] >> 16) + oy] = 1;
}

// zero the rows y of a width-wide plane whose mark rows[y + oy] is set
__global__ __launch_bounds__(256) void ZeroMarkedRows(float* __restrict__ plane, uint32_t width,
                                                      uint32_t height,
                                                      const uint8_t* __restrict__ rows,
                                                      uint32_t oy) {
  for (uint32_t y = blockIdx.x; y < height; y += gridDim.x) {
    if (!rows[y + oy]) continue;
    float* row = plane + size_t(y) * width;
    for (uint32_t x = threadIdx.x; x < width; x += 256) row[x] = 0.0f;
  }
}

// Model update of a scale > 0 outer iteration: model += the selection's
// component values convolved (circularly, as the FFT convolution of the
// reference does) with the scale's n x n shape kernel, by direct stamping.
// One workgroup per 64 x 64 output tile walks the selection in index order,
// keeps the components whose (wrapped) stamp reaches the tile, and sums
// m_c * k[y - y_c + n/2][x - x_c + n/2] per pixel in that order: a fixed
// summation order, so the result is reproducible.
constexpr uint32_t kStampTile = 64;
constexpr uint32_t kStampThreads = 256;
constexpr uint32_t kStampRows = kStampTile * kStampTile / kStampThreads;  // 16

// d in (-size, 2*size) -> d mod size
__device__ __forceinline__ uint32_t WrapDist(int32_t d, uint32_t size) {
  if (d < 0) d += int32_t(size);
  if (d >= int32_t(size)) d -= int32_t(size);
  return uint32_t(d);
}

// the tiles some component's n x n stamp reaches (circularly, as the
// stamping's hit test): a conservative byte map, so a tile no stamp reaches
// skips its walk over the selection
__device__ __forceinline__ void TileSpan(int32_t lo, int32_t hi, uint32_t size,
                                         uint32_t (&a)[2], uint32_t (&b)[2], int& k) {
  // [lo, hi] (hi - lo < size) as tile ranges, split where it wraps
  k = 0;
  if (lo < 0) {
    a[k] = uint32_t(lo + int32_t(size)) / kStampTile;
    b[k++] = (size - 1) / kStampTile;
    lo = 0;
  }
  if (hi >= int32_t(size)) {
    a[k] = 0;
    b[k++] = uint32_t(hi - int32_t(size)) / kStampTile;
    hi = int32_t(size) - 1;
  }
  a[k] = uint32_t(lo) / kStampTile;
  b[k++] = uint32_t(hi) / kStampTile;
}

// Per chunk of kStampThreads components (StampShapeModel's walk), the box
// its stamps cover, unwrapped: {x lo, x hi, y lo, y hi}; x lo > x hi when no
// component of the chunk is non-zero. One workgroup per chunk.
__global__ __launch_bounds__(256) void MarkStampTiles(const uint32_t* __restrict__ pos,
                                                      const float* __restrict__ m,
                                                      uint64_t n_sel, uint32_t n,
                                                      uint32_t width, uint32_t height,
                                                      uint32_t tiles_x,
                                                      uint8_t* __restrict__ mark,
                                                      int4* __restrict__ bounds) {
  const int32_t h = int32_t(n / 2);
  __shared__ int32_t red[4][256 / 64];
  int32_t bx0 = INT32_MAX, bx1 = INT32_MIN, by0 = INT32_MAX, by1 = INT32_MIN;
  const uint64_t c = blockIdx.x * uint64_t(256) + threadIdx.x;
  if (c < n_sel && m[c] != 0.0f) {
    const int32_t xc = int32_t(pos[c] & 0xffffu), yc = int32_t(pos[c] >> 16);
    bx0 = xc - h;
    bx1 = xc + h;
    by0 = yc - h;
    by1 = yc + h;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bx0 = min(bx0, __shfl_xor(bx0, off, 64));
    bx1 = max(bx1, __shfl_xor(bx1, off, 64));
    by0 = min(by0, __shfl_xor(by0, off, 64));
    by1 = max(by1, __shfl_xor(by1, off, 64));
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = bx0;
    red[1][wave] = bx1;
    red[2][wave] = by0;
    red[3][wave] = by1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < 256 / 64; ++w) {
      red[0][0] = min(red[0][0], red[0][w]);
      red[1][0] = max(red[1][0], red[1][w]);
      red[2][0] = min(red[2][0], red[2][w]);
      red[3][0] = max(red[3][0], red[3][w]);
    }
    bounds[blockIdx.x] = make_int4(red[0][0], red[1][0], red[2][0], red[3][0]);
  }
  {
    if (c >= n_sel || m[c] == 0.0f) return;
    const int32_t xc = int32_t(pos[c] & 0xffffu), yc = int32_t(pos[c] >> 16);
    uint32_t xa[2], xb[2], ya[2], yb[2];
    int nx, ny;
    TileSpan(xc - h, xc + h, width, xa, xb, nx);
    TileSpan(yc - h, yc + h, height, ya, yb, ny);
    for (int i = 0; i < ny; ++i)
      for (uint32_t ty = ya[i]; ty <= yb[i]; ++ty)
        for (int j = 0; j < nx; ++j)
          for (uint32_t tx = xa[j]; tx <= xb[j]; ++tx) mark[ty * tiles_x + tx] = 1;
  }
}

// a chunk's stamps miss the tile [t0, t0 + l) on one axis (a box that wraps
// around the plane never misses)
__device__ __forceinline__ bool StampMisses(int32_t lo, int32_t hi, uint32_t t0, uint32_t l,
                                            uint32_t size) {
  if (lo < 0 || hi >= int32_t(size)) return false;
  return hi < int32_t(t0) || lo >= int32_t(t0 + l);
}

__global__ __launch_bounds__(kStampThreads) void StampShapeModel(
    const uint32_t* __restrict__ pos, const float* __restrict__ m, uint64_t n_sel,
    const float* __restrict__ kern, uint32_t n, float* __restrict__ model,
    uint32_t width, uint32_t height, uint32_t tiles_x, const uint8_t* __restrict__ mark,
    const int4* __restrict__ bounds) {
  if (!mark[blockIdx.x]) return;
  __shared__ uint32_t list[kStampThreads];
  __shared__ uint32_t wave_count[kStampThreads / 64];
  __shared__ uint32_t n_list;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tx0 = (blockIdx.x % tiles_x) * kStampTile;
  const uint32_t ty0 = (blockIdx.x / tiles_x) * kStampTile;
  const uint32_t lx = min(kStampTile, width - tx0), ly = min(kStampTile, height - ty0);
  const uint32_t h = n / 2;
  const uint32_t px = tx0 + (tid % kStampTile);
  const uint32_t py0 = ty0 + tid / kStampTile;
  float acc[kStampRows];
#pragma unroll
  for (uint32_t r = 0; r < kStampRows; ++r) acc[r] = 0.0f;
  bool any = false;
  for (uint64_t base = 0; base < n_sel; base += kStampThreads) {
    // chunks whose stamps cannot reach this tile (components come in raster
    // order, so a chunk covers a few rows): skipped whole, uniformly
    if (bounds) {
      const int4 bb = bounds[base / kStampThreads];
      if (bb.x > bb.y || StampMisses(bb.x, bb.y, tx0, lx, width) ||
          StampMisses(bb.z, bb.w, ty0, ly, height))
        continue;
    }
    const uint64_t c = base + tid;
    bool hit = false;
    if (c < n_sel && m[c] != 0.0f) {
      const uint32_t pk = pos[c];
      const uint32_t xc = pk & 0xffffu, yc = pk >> 16;
      const uint32_t dx0 = WrapDist(int32_t(tx0) - int32_t(xc) + int32_t(h), width);
      const uint32_t dy0 = WrapDist(int32_t(ty0) - int32_t(yc) + int32_t(h), height);
      hit = (dx0 < n || dx0 + lx - 1 >= width) && (dy0 < n || dy0 + ly - 1 >= height);
    }
    // order-preserving compaction of the hits (wave order, then lane order)
    const uint64_t b = __ballot(hit);
    if (lane == 0) wave_count[wave] = uint32_t(__popcll(b));
    __syncthreads();
    uint32_t off = 0, total = 0;
    for (uint32_t w = 0; w < kStampThreads / 64; ++w) {
      if (w < wave) off += wave_count[w];
      total += wave_count[w];
    }
    if (hit) list[off + uint32_t(__popcll(b & ((uint64_t(1) << lane) - 1)))] = uint32_t(c - base);
    if (tid == 0) n_list = total;
    __syncthreads();
    const uint32_t cnt = n_list;
    any |= cnt != 0;
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint64_t cc = base + list[i];
      const uint32_t pk = pos[cc];
      const float v = m[cc];
      const uint32_t xc = pk & 0xffffu, yc = pk >> 16;
      const uint32_t dx = WrapDist(int32_t(px) - int32_t(xc) + int32_t(h), width);
      if (dx >= n || px >= width) continue;
      constexpr uint32_t kStep = kStampThreads / kStampTile;
      uint32_t dy = WrapDist(int32_t(py0) - int32_t(yc) + int32_t(h), height);
#pragma unroll
      for (uint32_t r = 0; r < kStampRows; ++r) {
        if (dy < n && py0 + r * kStep < height) acc[r] += v * kern[dy * n + dx];
        dy += kStep;
        if (dy >= height) dy -= height;
      }
    }
    __syncthreads();
  }
  if (!any || px >= width) return;
#pragma unroll
  for (uint32_t r = 0; r < kStampRows; ++r) {
    const uint32_t py = py0 + r * (kStampThreads / kStampTile);
    if (py < height) model[size_t(py) * width + px] += acc[r];
  }
}

}  // namespace rdl

extern "C" {

int rdl_subminor_model(rdl_subminor* h, uint32_t image_index, float* d_dest,
                       uint32_t dest_w, uint32_t dest_h, uint32_t ox,
                       uint32_t oy, int mode) {
  RDL_ARG_CHECK(h && d_dest, "NULL argument");
  RDL_ARG_CHECK(image_index < h->n_images || h->n_selected == 0,
                "image index out of range");
  RDL_ARG_CHECK(dest_w >= h->width + ox && dest_h >= h->height + oy,
                "destination too small");
  rdl_session* s = h->s;
  if (mode == 0)
    RDL_HIP_CHECK(hipMemsetAsync(d_dest, 0, size_t(dest_w) * dest_h * sizeof(float),
                                 s->stream));
  if (h->n_selected == 0) return RDL_OK;
  const unsigned grid = std::min<uint64_t>(4096, rdl::DivUp(h->n_selected, 256));
  rdl::ScatterModel<float><<<grid, 256, 0, s->stream>>>(
      h->d_pos, h->d_m + size_t(image_index) * h->n_selected, h->n_selected,
      d_dest, dest_w, ox, oy, mode == 1);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_subminor_model_masked(rdl_subminor* h, uint32_t image_index, float* d_dest,
                              uint32_t dest_w, uint32_t dest_h, const uint8_t* d_rows,
                              uint32_t oy) {
  RDL_ARG_CHECK(h && d_dest && d_rows, "NULL argument");
  RDL_ARG_CHECK(image_index < h->n_images || h->n_selected == 0,
                "image index out of range");
  RDL_ARG_CHECK(dest_w >= h->width && dest_h >= h->height, "destination too small");
  if (h->n_selected == 0) return RDL_OK;
  rdl_session* s = h->s;
  rdl::ZeroMarkedRows<<<std::min<uint32_t>(dest_h, 4096), 256, 0, s->stream>>>(
      d_dest, dest_w, dest_h, d_rows, oy);
  RDL_HIP_CHECK(hipGetLastError());
  const unsigned grid = std::min<uint64_t>(4096, rdl::DivUp(h->n_selected, 256));
  rdl::ScatterModel<float><<<grid, 256, 0, s->stream>>>(
      h->d_pos, h->d_m + size_t(image_index) * h->n_selected, h->n_selected, d_dest,
      dest_w, 0, 0, false);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_subminor_add_shape_model(rdl_subminor* h, uint32_t image_index,
                                 const float* d_kernel, uint32_t n, float* d_model,
                                 uint32_t width, uint32_t height) {
  RDL_ARG_CHECK(h && d_kernel && d_model, "NULL argument");
  RDL_ARG_CHECK(image_index < h->n_images || h->n_selected == 0,
                "image index out of range");
  RDL_ARG_CHECK(width == h->width && height == h->height, "model size differs");
  RDL_ARG_CHECK(n >= 1 && n % 2 == 1 && n <= width && n <= height,
                "shape kernel must be odd and no larger than the image");
  if (h->n_selected == 0) return RDL_OK;
  rdl_session* s = h->s;
  const uint32_t tiles_x = rdl::DivUp(width, rdl::kStampTile);
  const uint32_t tiles_y = rdl::DivUp(height, rdl::kStampTile);
  {
    // algorithmic bytes: the selection read per tile is cached; count the
    // model read-modify-write of the whole plane
    rdl::ScopedTiming t(s, "stamp_model", 8.0 * double(width) * height);
    const size_t n_tiles = size_t(tiles_x) * tiles_y;
    const size_t n_chunks = rdl::DivUp(h->n_selected, rdl::kStampThreads);
    const size_t mark_bytes = (n_tiles + 15) / 16 * 16;
    RDL_TRY(rdl::Grow(&h->stamp_mark, &h->stamp_mark_bytes,
                      mark_bytes + n_chunks * sizeof(int4), s->stream));
    uint8_t* mark = static_cast<uint8_t*>(h->stamp_mark);
    int4* bounds = reinterpret_cast<int4*>(mark + mark_bytes);
    RDL_HIP_CHECK(hipMemsetAsync(mark, 0, n_tiles, s->stream));
    const float* mi = h->d_m + size_t(image_index) * h->n_selected;
    static_assert(rdl::kStampThreads == 256, "one MarkStampTiles workgroup per chunk");
    rdl::MarkStampTiles<<<unsigned(n_chunks), 256, 0, s->stream>>>(
        h->d_pos, mi, h->n_selected, n, width, height, tiles_x, mark, bounds);
    // RDL_STAMP_BOUNDS=0: every tile walks every chunk (comparison)
    static const bool bounds_on = [] {
      const char* e = std::getenv("RDL_STAMP_BOUNDS");
      return !(e && e[0] == '0');
    }();
    rdl::StampShapeModel<<<tiles_x * tiles_y, rdl::kStampThreads, 0, s->stream>>>(
        h->d_pos, mi, h->n_selected, d_kernel, n, d_model, width, height, tiles_x, mark,
        bounds_on ? bounds : nullptr);
  }
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_subminor_model_rows(rdl_subminor* h, uint32_t image_index,
                            uint8_t* d_rows, uint32_t n_rows, uint32_t oy) {
  RDL_ARG_CHECK(h && d_rows, "NULL argument");
  RDL_ARG_CHECK(image_index < h->n_images || h->n_selected == 0,
                "image index out of range");
  RDL_ARG_CHECK(n_rows >= h->height + oy, "row mask too short");
  rdl_session* s = h->s;
  RDL_HIP_CHECK(hipMemsetAsync(d_rows, 0, n_rows, s->stream));
  if (h->n_selected == 0) return RDL_OK;
  const unsigned grid = std::min<uint64_t>(4096, rdl::DivUp(h->n_selected, 256));
  rdl::MarkModelRows<<<grid, 256, 0, s->stream>>>(
      h->d_pos, h->d_m + size_t(image_index) * h->n_selected, h->n_selected, d_rows,
      oy);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_subminor_model_f64(rdl_subminor* h, uint32_t image_index,
                           double* d_dest, uint32_t dest_w, uint32_t dest_h,
                           uint32_t ox, uint32_t oy) {
  RDL_ARG_CHECK(h && d_dest, "NULL argument");
  RDL_ARG_CHECK(image_index < h->n_images || h->n_selected == 0,
                "image index out of range");
  RDL_ARG_CHECK(dest_w >= h->width + ox && dest_h >= h->height + oy,
                "destination too small");
  rdl_session* s = h->s;
  RDL_HIP_CHECK(hipMemsetAsync(d_dest, 0, size_t(dest_w) * dest_h * sizeof(double),
                               s->stream));
  if (h->n_selected == 0) return RDL_OK;
  const unsigned grid = std::min<uint64_t>(4096, rdl::DivUp(h->n_selected, 256));
  rdl::ScatterModel<double><<<grid, 256, 0, s->stream>>>(
      h->d_pos, h->d_m + size_t(image_index) * h->n_selected, h->n_selected,
      d_dest, dest_w, ox, oy, 0);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_subminor_update_mask(rdl_subminor* h, uint8_t* d_mask) {
  RDL_ARG_CHECK(h && d_mask, "NULL argument");
  if (h->n_selected == 0) return RDL_OK;
  const uint32_t grid = uint32_t((h->n_selected + 255) / 256);
  rdl::UpdateMaskKernel<<<grid, 256, 0, h->s->stream>>>(h->d_pos, h->d_m, h->n_selected,
                                                       h->n_images, h->width, d_mask);
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

int rdl_subminor_get(rdl_subminor* h, uint32_t* h_positions, float* h_models,
                     uint64_t capacity) {
  RDL_ARG_CHECK(h, "NULL argument");
  const uint64_t n = std::min(capacity, h->n_selected);
  if (n == 0) return RDL_OK;
  if (h_positions)
    RDL_HIP_CHECK(hipMemcpyAsync(h_positions, h->d_pos, n * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, h->s->stream));
  if (h_models)
    for (uint32_t k = 0; k < h->n_images; ++k)
      RDL_HIP_CHECK(hipMemcpyAsync(h_models + k * n, h->d_m + k * h->n_selected,
                                   n * sizeof(float), hipMemcpyDeviceToHost,
                                   h->s->stream));
  RDL_HIP_CHECK(hipStreamSynchronize(h->s->stream));
  return RDL_OK;
}

}  // extern "C"
