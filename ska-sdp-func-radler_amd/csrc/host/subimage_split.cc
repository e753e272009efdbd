// Line references: the reference's cpp/algorithms/parallel_deconvolution.cc.
#include "subimage_split.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <exception>
#include <memory>
#include <new>
#include <thread>

#include "dijkstra_splitter.h"
#include "host_profile.h"

namespace radler::algorithms {

size_t NearestPsfIndex(const std::vector<PsfOffset>& psf_offsets, size_t x,
                       size_t y) noexcept {
  if (psf_offsets.empty()) return 0;
  auto distance = [x, y](const PsfOffset& p) {
    const ssize_t dx = ssize_t(p.x) - ssize_t(x);
    const ssize_t dy = ssize_t(p.y) - ssize_t(y);
    return size_t(dx * dx) + size_t(dy * dy);
  };
  return std::min_element(psf_offsets.begin(), psf_offsets.end(),
                          [&](const PsfOffset& a, const PsfOffset& b) {
                            return distance(a) < distance(b);
                          }) -
         psf_offsets.begin();
}

namespace {

// Run f(0..n-1) on up to `threads` host threads (work items claimed in order).
template <typename F>
void ParallelFor(size_t n, size_t threads, F&& f) {
  threads = std::max<size_t>(1, std::min(threads, n));
  if (threads == 1) {
    for (size_t i = 0; i != n; ++i) f(i);
    return;
  }
  std::atomic<size_t> next{0};
  std::vector<std::exception_ptr> errors(threads);
  std::vector<std::thread> pool;
  for (size_t t = 0; t != threads; ++t)
    pool.emplace_back([&, t] {
      try {
        for (size_t i = next++; i < n; i = next++) f(i);
      } catch (...) {
        errors[t] = std::current_exception();
      }
    });
  for (std::thread& th : pool) th.join();
  for (std::exception_ptr& e : errors)
    if (e) std::rethrow_exception(e);
}

size_t HostThreads() {
  const size_t hw = std::thread::hardware_concurrency();
  return std::max<size_t>(1, std::min<size_t>(hw ? hw : 1, 16));
}

// The gw - 1 vertical and gh - 1 horizontal dividers: searches in disjoint bands.
void MakeDividers(const float* image, size_t width, size_t height, size_t gw, size_t gh,
                  float* dividing_v, float* dividing_h) {
  prof::Section p("split.divide");
  const size_t avg_w = width / gw, avg_h = height / gh;
  math::DijkstraSplitter splitter(width, height);
  ParallelFor((gw - 1) + (gh - 1), HostThreads(), [&](size_t k) {
    if (k + 1 < gw) {
      const size_t mid = width * (k + 1) / gw;
      splitter.DivideVertically(image, dividing_v, mid - avg_w / 4, mid + avg_w / 4);
    } else {
      const size_t mid = height * (k + 2 - gw) / gh;
      splitter.DivideHorizontally(image, dividing_h, mid - avg_h / 4, mid + avg_h / 4);
    }
  });
}

// An area between dividers: [lo, hi) of columns per row (vertical), or the transpose.
struct Runs {
  std::vector<uint32_t> lo, hi;
  size_t start = 0, extent = 0;  // x, width (or y, height) of the area
};

// Flood{Vertical,Horizontal}Area from `centre`: over zeros, plus the low side's divider.
Runs FloodAreaRuns(const float* div, bool vertical, size_t width, size_t height,
                   size_t centre) {
  const size_t n = vertical ? height : width;    // runs
  const size_t len = vertical ? width : height;  // along a run
  const size_t stride = vertical ? 1 : width;    // step along a run
  const size_t across = vertical ? width : 1;    // step between runs
  Runs r;
  r.lo.resize(n);
  r.hi.resize(n);
  size_t first = len, last = 0;
  for (size_t j = 0; j != n; ++j) {
    const float* line = div + j * across;
    int64_t i = int64_t(centre);
    for (; i >= 0 && line[i * stride] == 0.0f; --i) {
    }
    for (; i >= 0 && line[i * stride] != 0.0f; --i) {
    }
    const size_t lo = size_t(i + 1);
    size_t hi = centre + 1;
    for (; hi < len && line[hi * stride] == 0.0f; ++hi) {
    }
    r.lo[j] = uint32_t(lo);
    r.hi[j] = uint32_t(hi);
    first = std::min(first, lo);
    last = std::max(last, hi);
  }
  r.start = first;
  r.extent = last < first ? 0 : last - first;
  return r;
}

// GetBoundingMask of a cell (the overlap of its two areas): the box and both masks.
void BoundCell(size_t width, size_t height, const Runs& col, const Runs& row,
               const bool* user_mask, SubImage& sub) {
  auto inside = [&](size_t x, size_t y) {
    return x >= col.lo[y] && x < col.hi[y] && y >= row.lo[x] && y < row.hi[x];
  };
  // rows that can hold the cell: the row area's extent over the column's x range
  size_t y_from = height, y_to = 0;
  for (size_t x = col.start; x < col.start + col.extent; ++x) {
    y_from = std::min<size_t>(y_from, row.lo[x]);
    y_to = std::max<size_t>(y_to, row.hi[x]);
  }
  size_t x_lo = col.extent + col.start, y_lo = height, x_hi = 0, y_hi = 0;
  for (size_t y = y_from; y < y_to; ++y)
    for (size_t x = col.lo[y]; x < col.hi[y]; ++x)
      if (y >= row.lo[x] && y < row.hi[x]) {
        x_lo = std::min(x_lo, x);
        x_hi = std::max(x_hi, x);
        y_lo = std::min(y_lo, y);
        y_hi = y;
      }
  size_t sw = 0, sh = 0;
  if (x_hi >= x_lo) {
    sw = x_hi + 1 - x_lo;
    sh = y_hi + 1 - y_lo;
  }
  // even images keep even subimages: one more column/row (to the left/top
  // when the right/bottom edge would leave the image), masked out
  // (dijkstra_splitter.cc GetBoundingMask)
  size_t ext_col = SIZE_MAX, ext_row = SIZE_MAX;
  if (width % 2 == 0 && sw % 2 != 0) {
    ++sw;
    ext_col = sw + x_lo >= width ? --x_lo : x_lo + sw - 1;
  }
  if (height % 2 == 0 && sh % 2 != 0) {
    ++sh;
    ext_row = sh + y_lo >= height ? --y_lo : y_lo + sh - 1;
  }
  sub.x = x_lo;
  sub.y = y_lo;
  sub.width = sw;
  sub.height = sh;
  sub.mask.assign(sw * sh, false);
  for (size_t y = 0; y != sh; ++y) {
    const size_t gy_ = y + y_lo;
    if (gy_ == ext_row) continue;
    const size_t from = std::max<size_t>(col.lo[gy_], x_lo);
    const size_t to = std::min<size_t>(col.hi[gy_], x_lo + sw);
    for (size_t gx_ = from; gx_ < to; ++gx_)
      if (gx_ != ext_col && inside(gx_, gy_)) sub.mask[y * sw + gx_ - x_lo] = true;
  }
  sub.boundary_mask = sub.mask;
  if (user_mask)
    for (size_t y = 0; y != sh; ++y)
      for (size_t x = 0; x != sw; ++x)
        sub.mask[y * sw + x] =
            sub.mask[y * sw + x] && user_mask[(y + sub.y) * width + x + sub.x];
}

}  // namespace

// MakeSubImages (parallel_deconvolution.cc:57-166): Dijkstra dividers through
// the integrated image, then per grid cell the overlap of its vertical and
// horizontal areas; the subimage mask is that overlap, ANDed with the user
// clean mask when there is one.
//
// Same result as DijkstraSplitter's FloodVerticalArea / FloodHorizontalArea /
// GetBoundingMask sequence (the reference's), computed as intervals: every
// row of a vertical area is one run [left, right) of columns and every column
// of a horizontal area one run [top, bottom) of rows, so the overlap of a
// cell needs no full-image masks. The areas are independent and run
// concurrently, as do the cells.
std::vector<SubImage> MakeSubImages(const std::vector<float>& image, size_t width,
                                    size_t height, const bool* user_mask,
                                    const std::vector<PsfOffset>& psf_offsets,
                                    const Settings& settings,
                                    std::vector<size_t>& psf_indices) {
  const size_t gw = settings.parallel.grid_width, gh = settings.parallel.grid_height;
  // the divider planes: zero pages from calloc (the searches write only
  // their bands and the floods mostly read zeros; value-initialised vectors
  // wrote 2 x 4 bytes per pixel first, ~0.1 s of the split at 8192^2)
  auto zero_plane = [&] {
    std::unique_ptr<float, decltype(&std::free)> p(
        static_cast<float*>(std::calloc(width * height, sizeof(float))), &std::free);
    if (!p) throw std::bad_alloc();
    return p;
  };
  auto dividing_v = zero_plane(), dividing_h = zero_plane();
  MakeDividers(image.data(), width, height, gw, gh, dividing_v.get(), dividing_h.get());
  prof::Section p_masks("split.masks");
  std::vector<Runs> columns(gw), rows(gh);
  ParallelFor(gw + gh, HostThreads(), [&](size_t k) {
    if (k < gw)
      columns[k] = FloodAreaRuns(dividing_v.get(), true, width, height,
                                 k * width / gw + width / gw / 2);
    else
      rows[k - gw] = FloodAreaRuns(dividing_h.get(), false, width, height,
                                   (k - gw) * height / gh + height / gh / 2);
  });
  dividing_v.reset();
  dividing_h.reset();
  std::vector<SubImage> subs(gw * gh);
  ParallelFor(subs.size(), HostThreads(), [&](size_t index) {
    subs[index].index = index;
    BoundCell(width, height, columns[index % gw], rows[index / gw], user_mask,
              subs[index]);
  });
  for (const SubImage& sub : subs)
    psf_indices.push_back(NearestPsfIndex(psf_offsets, sub.x + sub.width / 2,
                                          sub.y + sub.height / 2));
  return subs;
}

}  // namespace radler::algorithms
