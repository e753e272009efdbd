// The sub-minor loop's selection: findPeakPositions / MakeSets
// (subminor_loop.cc:143-184). The pixels of the border box whose integrated
// value passes the threshold, compacted into a row-major list (packed
// y<<16|x), and their N_img residual values: the order the reference's nested
// x/y loops produce. Three schemes with the same result: the sparse two-phase
// selection (the default: SelLocal or SelLocalQuad, SelScan, SelPlace), the
// single pass with look-back (SelSinglePass) and count + scan + scatter
// (SelCount, SelScan, SelScatter), the last two kept for comparison
// (RDL_SUBMINOR_SELECT).
#include "subminor_internal.h"

namespace rdl {

constexpr uint32_t kChunk = 2048;  // box pixels per selection workgroup
constexpr uint32_t kSelThreads = 256;

struct SelArgs {
  const float* residuals;
  const uint8_t* mask;
  uint32_t width, height, n;  // n = width*height
  uint32_t xs, xe, ys, ye, bw;
  uint64_t box_pixels;
  rdl_integration integ;
  float threshold;
  int32_t allow_negative;
  const float* rms;  // RMS factor image (W x H) or nullptr
};

// A thread's box position, advanced by a fixed stride without dividing (a
// 64-bit divide per pixel made the selection passes ALU-bound).
struct BoxWalker {
  uint64_t b;
  uint32_t x, y;  // inside the box
  __device__ BoxWalker(const SelArgs& a, uint64_t b0)
      : b(b0), x(uint32_t(b0 % a.bw)), y(uint32_t(b0 / a.bw)) {}
  __device__ void Advance(const SelArgs& a, uint32_t stride) {
    b += stride;
    x += stride;
    while (x >= a.bw) {
      x -= a.bw;
      ++y;
    }
  }
};

// the selection test of pixel idx whose first image's residual v0 the
// caller loaded (so a thread's loads can all be in flight at once)
__device__ __forceinline__ bool SelectedValue(const SelArgs& a, uint32_t idx, float v0) {
  if (a.mask && !a.mask[idx]) return false;
  float v = IntegratePixel(a.integ, [&](uint32_t k) {
    return k == 0 ? v0 : a.residuals[size_t(k) * a.n + idx];
  });
  if (a.rms) v *= a.rms[idx];  // integratedScratch *= rms (subminor_loop.cc:147-149)
  const float value = a.allow_negative ? fabsf(v) : v;
  return value >= a.threshold;
}

__device__ __forceinline__ bool Selected(const SelArgs& a, const BoxWalker& w,
                                         uint32_t& idx) {
  if (w.b >= a.box_pixels) return false;
  idx = (a.ys + w.y) * a.width + a.xs + w.x;
  if (a.mask && !a.mask[idx]) return false;
  float v = IntegratePixel(
      a.integ, [&](uint32_t k) { return a.residuals[size_t(k) * a.n + idx]; });
  if (a.rms) v *= a.rms[idx];  // integratedScratch *= rms (subminor_loop.cc:147-149)
  const float value = a.allow_negative ? fabsf(v) : v;
  return value >= a.threshold;
}

__global__ __launch_bounds__(kSelThreads) void SelCount(SelArgs a,
                                                        uint32_t* counts) {
  __shared__ uint32_t lds[kSelThreads / 64];
  uint32_t c = 0;
  const uint64_t base = uint64_t(blockIdx.x) * kChunk;
  BoxWalker bw(a, base + threadIdx.x);
  constexpr uint32_t kItems = kChunk / kSelThreads;
  uint32_t idx[kItems];
  float v0[kItems];
#pragma unroll
  for (uint32_t i = 0; i < kItems; ++i) {
    idx[i] = bw.b < a.box_pixels ? (a.ys + bw.y) * a.width + a.xs + bw.x : 0xffffffffu;
    bw.Advance(a, kSelThreads);
  }
#pragma unroll
  for (uint32_t i = 0; i < kItems; ++i)
    v0[i] = a.residuals[idx[i] == 0xffffffffu ? 0u : idx[i]];
#pragma unroll
  for (uint32_t i = 0; i < kItems; ++i)
    c += (idx[i] != 0xffffffffu && SelectedValue(a, idx[i], v0[i])) ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < kSelThreads / 64; ++w) t += lds[w];
    counts[blockIdx.x] = t;
  }
}

// Exclusive scan of the chunk counts in one workgroup; writes the total.
// Thread t owns the contiguous segment [t seg, (t + 1) seg): sums it, one
// block scan of the 1024 sums, then rewrites its segment as offsets.
__global__ __launch_bounds__(1024) void SelScan(uint32_t* counts, uint32_t n,
                                                uint64_t* total, uint64_t* total_host) {
  __shared__ uint64_t lds[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t seg = (n + 1023) / 1024;
  const uint32_t lo = min(n, t * seg), hi = min(n, lo + seg);
  uint64_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += counts[i];
  lds[t] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    const uint64_t v = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += v;
    __syncthreads();
  }
  uint64_t run = lds[t] - sum;  // exclusive
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t c = counts[i];
    counts[i] = uint32_t(run);
    run += c;
  }
  if (t == 1023) {
    *total = lds[1023];
    *total_host = lds[1023];  // the host's copy (mapped memory, no read-back copy)
  }
}

__global__ __launch_bounds__(kSelThreads) void SelScatter(
    SelArgs a, const uint32_t* offsets, uint32_t n_img, uint64_t n_sel,
    uint32_t* pos, float* r) {
  __shared__ uint32_t wave_tot[kSelThreads / 64];
  const uint64_t base = uint64_t(blockIdx.x) * kChunk;
  uint32_t running = offsets[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  BoxWalker bw(a, base + threadIdx.x);
  for (uint32_t j0 = 0; j0 < kChunk; j0 += kSelThreads) {
    uint32_t idx = 0;
    const bool sel = Selected(a, bw, idx);
    bw.Advance(a, kSelThreads);
    const uint64_t ballot = __ballot(sel);
    const uint32_t before = __popcll(ballot & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(ballot);
    __syncthreads();
    uint32_t woff = 0;
    for (int w = 0; w < wave; ++w) woff += wave_tot[w];
    uint32_t step = 0;
    for (uint32_t w = 0; w < kSelThreads / 64; ++w) step += wave_tot[w];
    if (sel) {
      const uint64_t o = running + woff + before;
      const uint32_t x = idx % a.width, y = idx / a.width;
      pos[o] = (y << 16) | x;
      for (uint32_t k = 0; k < n_img; ++k)
        r[size_t(k) * n_sel + o] = a.residuals[size_t(k) * a.n + idx];
    }
    running += step;
    __syncthreads();
  }
}

// Single-pass selection (replaces SelCount + SelScan + SelScatter): each
// workgroup takes the next chunk in launch order (a ticket), flags its
// pixels once, publishes its count, and finds its output offset by
// decoupled look-back over its predecessors' published counts / prefixes
// (status words {flag, value}, single-copy-atomic 8-byte stores; flag 1 =
// the chunk's count, 2 = the inclusive prefix). Positions only; the residual
// values follow in SelGather once the host knows the count. One read of the
// box instead of two, no scan launch. Output order = ascending box order,
// as the three-kernel path.
constexpr uint32_t kSpThreads = 512;
constexpr uint32_t kSelItems = 16;
constexpr uint32_t kSpChunk = kSpThreads * kSelItems;  // box pixels per workgroup
constexpr uint64_t kStatusAggregate = uint64_t(1) << 32;
constexpr uint64_t kStatusPrefix = uint64_t(2) << 32;

__global__ __launch_bounds__(kSpThreads) void SelSinglePass(SelArgs a, uint32_t* ticket,
                                                             uint64_t* status,
                                                             uint32_t n_chunks, uint32_t* pos,
                                                             uint64_t* total,
                                                             uint32_t* failed,
                                                             uint64_t spin_limit) {
  __shared__ uint32_t chunk_s;
  __shared__ uint32_t wave_tot[kSelItems][kSpThreads / 64];
  __shared__ uint32_t excl_s;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // ticket: chunks in the order workgroups start (NULL: blockIdx, which the
  // dispatcher hands out in order on each XCD)
  if (tid == 0) chunk_s = ticket ? atomicAdd(ticket, 1u) : blockIdx.x;
  __syncthreads();
  const uint32_t b = chunk_s;
  const uint64_t base = uint64_t(b) * kSpChunk;
  uint64_t ballots[kSelItems];
  uint32_t idx[kSelItems];
  BoxWalker bw(a, base + tid);
  float v0[kSelItems];
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i) {
    idx[i] = bw.b < a.box_pixels ? (a.ys + bw.y) * a.width + a.xs + bw.x : 0xffffffffu;
    bw.Advance(a, kSpThreads);
  }
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i)  // every load in flight at once
    v0[i] = a.residuals[idx[i] == 0xffffffffu ? 0u : idx[i]];
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i) {
    const bool sel = idx[i] != 0xffffffffu && SelectedValue(a, idx[i], v0[i]);
    ballots[i] = __ballot(sel);
    if (lane == 0) wave_tot[i][wave] = uint32_t(__popcll(ballots[i]));
  }
  __syncthreads();
  uint32_t count = 0;
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i)
#pragma unroll
    for (uint32_t w = 0; w < kSpThreads / 64; ++w) count += wave_tot[i][w];
  if (wave == 0) {
    uint64_t excl = 0;
    if (b == 0) {
      if (lane == 0)
        __hip_atomic_store(&status[0], kStatusPrefix | count, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (lane == 0)
        __hip_atomic_store(&status[b], kStatusAggregate | count, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      // look back 64 predecessors at a time (lane l: chunk b - 1 - l)
      int64_t p = int64_t(b) - 1 - int64_t(lane);
      uint64_t spins = 0;
      while (true) {
        uint64_t st = p >= 0 ? __hip_atomic_load(&status[p], __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT)
                             : kStatusPrefix;  // before chunk 0: prefix 0
        // every predecessor publishes its count before it looks back
        while (!__all((st >> 32) != 0u)) {
          __builtin_amdgcn_s_sleep(1);
          if ((st >> 32) == 0u)
            st = __hip_atomic_load(&status[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (++spins > spin_limit) break;  // never expected; ends the wave
        }
        const uint64_t pm = __ballot((st >> 32) == 2u);
        const uint32_t v = uint32_t(st);
        if (pm) {
          const uint32_t first = uint32_t(__builtin_ctzll(pm));  // nearest prefix
          uint64_t part = lane <= first ? uint64_t(v) : 0ull;
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
          excl += part;
          break;
        }
        uint64_t part = v;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
        excl += part;
        p -= 64;
        if (spins > spin_limit) break;
      }
      // a predecessor never published (never expected): the prefix is wrong,
      // so the selection is reported failed rather than silently corrupt
      if (spins > spin_limit && lane == 0) atomicOr(failed, 1u);
      if (lane == 0)
        __hip_atomic_store(&status[b], kStatusPrefix | uint32_t(excl + count),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) {
      excl_s = uint32_t(excl);
      if (b == n_chunks - 1) *total = excl + count;
    }
  }
  __syncthreads();
  uint32_t o = excl_s;
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i) {
    uint32_t woff = 0, step = 0;
#pragma unroll
    for (uint32_t w = 0; w < kSpThreads / 64; ++w) {
      woff += w < wave ? wave_tot[i][w] : 0u;
      step += wave_tot[i][w];
    }
    if ((ballots[i] >> lane) & 1ull) {
      const uint32_t before = uint32_t(__popcll(ballots[i] & ((1ull << lane) - 1ull)));
      const uint32_t x = idx[i] % a.width, y = idx[i] / a.width;
      pos[o + woff + before] = (y << 16) | x;
    }
    o += step;
  }
}

// Sparse two-phase selection (the default): SelLocal flags each chunk's
// pixels once (the single pass's loads and tests) and stores the chunk's
// count and its selected positions, ascending, in the chunk's own slot of
// `local`; SelScan turns the counts into offsets; SelPlace moves every
// non-empty chunk's positions to its offset. No workgroup waits for another
// (the single pass's look-back chained the chunks), and a selection is a few
// thousand pixels, so the second pass touches a few hundred chunks.
__global__ __launch_bounds__(kSpThreads) void SelLocal(SelArgs a, uint32_t* __restrict__ counts,
                                                       uint32_t* __restrict__ local) {
  __shared__ uint32_t wave_tot[kSelItems][kSpThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  const uint64_t base = uint64_t(b) * kSpChunk;
  uint64_t ballots[kSelItems];
  uint32_t idx[kSelItems];
  BoxWalker bw(a, base + tid);
  float v0[kSelItems];
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i) {
    idx[i] = bw.b < a.box_pixels ? (a.ys + bw.y) * a.width + a.xs + bw.x : 0xffffffffu;
    bw.Advance(a, kSpThreads);
  }
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i)  // every load in flight at once
    v0[i] = a.residuals[idx[i] == 0xffffffffu ? 0u : idx[i]];
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i) {
    const bool sel = idx[i] != 0xffffffffu && SelectedValue(a, idx[i], v0[i]);
    ballots[i] = __ballot(sel);
    if (lane == 0) wave_tot[i][wave] = uint32_t(__popcll(ballots[i]));
  }
  __syncthreads();
  uint32_t count = 0;
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i)
#pragma unroll
    for (uint32_t w = 0; w < kSpThreads / 64; ++w) count += wave_tot[i][w];
  if (tid == 0) counts[b] = count;
  if (count == 0) return;
  uint32_t* out = local + base;
  uint32_t o = 0;
#pragma unroll
  for (uint32_t i = 0; i < kSelItems; ++i) {
    uint32_t woff = 0, step = 0;
#pragma unroll
    for (uint32_t w = 0; w < kSpThreads / 64; ++w) {
      woff += w < wave ? wave_tot[i][w] : 0u;
      step += wave_tot[i][w];
    }
    if ((ballots[i] >> lane) & 1ull) {
      const uint32_t before = uint32_t(__popcll(ballots[i] & ((1ull << lane) - 1ull)));
      const uint32_t x = idx[i] % a.width, y = idx[i] / a.width;
      out[o + woff + before] = (y << 16) | x;
    }
    o += step;
  }
}

// SelLocal with 16-byte loads (rows whose width is a multiple of 4, one
// image with the identity integration, no RMS weights): a workgroup takes
// `rpb` box rows, each as `ipr` items of 512 float4 (items of a row in
// order, rows in order: box order), so the selection costs a peak search's
// read. A lane's 4-pixel flags are ranked across the wave from three
// ballots of its count's bits.
constexpr uint32_t kQuadItems = 8;
constexpr uint32_t kQuadChunk = kSpThreads * kQuadItems * 4;  // pixel slots per chunk

__global__ __launch_bounds__(kSpThreads) void SelLocalQuad(SelArgs a, uint32_t ipr, uint32_t rpb,
                                                           uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ local) {
  __shared__ uint32_t wave_tot[kQuadItems][kSpThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t b = blockIdx.x;
  const uint32_t y0 = a.ys + b * rpb;
  const uint32_t y1 = min(a.ye, y0 + rpb);
  const uint32_t q0 = a.xs >> 2, q1 = (a.xe + 3) >> 2;
  const uint64_t lower = (uint64_t(1) << lane) - 1ull;
  float4 v[kQuadItems];
  uint32_t mk[kQuadItems];
#pragma unroll
  for (uint32_t i = 0; i < kQuadItems; ++i) {  // every load in flight at once
    const uint32_t y = y0 + i / ipr, q = q0 + (i % ipr) * kSpThreads + tid;
    const bool in = y < y1 && q < q1;
    v[i] = in ? reinterpret_cast<const float4*>(a.residuals + size_t(y) * a.width)[q]
              : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    mk[i] = in ? 0x01010101u : 0u;
    if (in && a.mask) mk[i] = reinterpret_cast<const uint32_t*>(a.mask + size_t(y) * a.width)[q];
  }
  uint32_t m4[kQuadItems], pre[kQuadItems];
  uint32_t any_m = 0u;
#pragma unroll
  for (uint32_t i = 0; i < kQuadItems; ++i) {
    const uint32_t q = q0 + (i % ipr) * kSpThreads + tid;
    const float vv[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t x = 4 * q + j;
      const float value = a.allow_negative ? fabsf(vv[j]) : vv[j];
      const bool sel = ((mk[i] >> (8 * j)) & 0xffu) && x >= a.xs && x < a.xe &&
                       value >= a.threshold;
      m |= sel ? (1u << j) : 0u;
    }
    m4[i] = m;
    any_m |= m;
  }
  // a selection is sparse: most waves select nothing and skip the ranking
  if (__any(any_m != 0u)) {
#pragma unroll
    for (uint32_t i = 0; i < kQuadItems; ++i) {
      const uint32_t c = uint32_t(__popc(m4[i]));
      const uint64_t b0 = __ballot(c & 1u), b1 = __ballot(c & 2u), b2 = __ballot(c & 4u);
      pre[i] = uint32_t(__popcll(b0 & lower) + 2 * __popcll(b1 & lower) + 4 * __popcll(b2 & lower));
      if (lane == 0)
        wave_tot[i][wave] = uint32_t(__popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2));
    }
  } else {
#pragma unroll
    for (uint32_t i = 0; i < kQuadItems; ++i) {
      pre[i] = 0u;
      if (lane == 0) wave_tot[i][wave] = 0u;
    }
  }
  __syncthreads();
  uint32_t count = 0;
#pragma unroll
  for (uint32_t i = 0; i < kQuadItems; ++i)
#pragma unroll
    for (uint32_t w = 0; w < kSpThreads / 64; ++w) count += wave_tot[i][w];
  if (tid == 0) counts[b] = count;
  if (count == 0) return;
  uint32_t* out = local + uint64_t(b) * kQuadChunk;
  uint32_t o = 0;
#pragma unroll
  for (uint32_t i = 0; i < kQuadItems; ++i) {
    uint32_t woff = 0, step = 0;
#pragma unroll
    for (uint32_t w = 0; w < kSpThreads / 64; ++w) {
      woff += w < wave ? wave_tot[i][w] : 0u;
      step += wave_tot[i][w];
    }
    if (m4[i]) {
      const uint32_t y = y0 + i / ipr, q = q0 + (i % ipr) * kSpThreads + tid;
      uint32_t k = o + woff + pre[i];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j)
        if ((m4[i] >> j) & 1u) out[k++] = (y << 16) | (4 * q + j);
    }
    o += step;
  }
}

// chunk b's positions (offsets[b] .. offsets[b + 1], the last to *total)
__global__ __launch_bounds__(256) void SelPlace(const uint32_t* __restrict__ offsets,
                                                uint32_t n_chunks,
                                                const uint64_t* __restrict__ total,
                                                const uint32_t* __restrict__ local,
                                                uint32_t chunk_slots,
                                                uint32_t* __restrict__ pos) {
  const uint32_t b = blockIdx.x;
  const uint32_t off = offsets[b];
  const uint32_t end = b + 1 < n_chunks ? offsets[b + 1] : uint32_t(*total);
  const uint32_t* src = local + uint64_t(b) * chunk_slots;
  for (uint32_t k = threadIdx.x; off + k < end; k += 256) pos[off + k] = src[k];
}

// the selected pixels' residual values, [image][n_sel]
__global__ __launch_bounds__(256) void SelGather(const float* residuals, uint32_t width,
                                                 uint32_t n, const uint32_t* pos,
                                                 uint64_t n_sel, uint32_t n_img, float* r) {
  for (uint64_t j = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; j < n_sel;
       j += uint64_t(gridDim.x) * blockDim.x) {
    const uint32_t p = pos[j];
    const uint32_t idx = (p >> 16) * width + (p & 0xffffu);
    for (uint32_t k = 0; k < n_img; ++k) r[k * n_sel + j] = residuals[size_t(k) * n + idx];
  }
}

int RunSelection(rdl_subminor* h, const float* d_residuals, const rdl_subminor_params* p,
                 uint64_t* n_sel_out) {
  rdl_session* s = h->s;
  hipStream_t st = s->stream;
  SelArgs sa{};
  sa.residuals = d_residuals;
  sa.mask = p->d_mask;
  sa.width = p->width;
  sa.height = p->height;
  sa.n = p->width * p->height;
  sa.xs = p->h_border;
  sa.xe = std::max<int64_t>(sa.xs, int64_t(p->width) - int64_t(p->h_border));
  sa.ys = p->v_border;
  sa.ye = std::max<int64_t>(sa.ys, int64_t(p->height) - int64_t(p->v_border));
  sa.xe = std::min(sa.xe, p->width);
  sa.ye = std::min(sa.ye, p->height);
  sa.xs = std::min(sa.xs, sa.xe);
  sa.ys = std::min(sa.ys, sa.ye);
  sa.bw = std::max<uint32_t>(1, sa.xe - sa.xs);
  sa.box_pixels = uint64_t(sa.xe - sa.xs) * (sa.ye - sa.ys);
  sa.integ = p->integ;
  sa.threshold = p->threshold;
  sa.allow_negative = p->allow_negative;
  sa.rms = p->d_rms;
  // the sparse selection's 16-byte-load variant: rows of whole float4
  // (width % 4 == 0), at most 16 items of 512 float4 per row
  const uint32_t quads_per_row = ((sa.xe + 3) >> 2) - (sa.xs >> 2);
  const uint32_t quad_ipr = std::max<uint32_t>(1, DivUp(quads_per_row, kSpThreads));
  const bool quad = h->select_passes == 0 && h->select_quad && p->width % 4 == 0 &&
                    p->integ.copy_fast_path && !p->d_rms && sa.box_pixels > 0 &&
                    quad_ipr <= kQuadItems;
  const uint32_t quad_rpb = kQuadItems / quad_ipr;
  const uint32_t n_chunks =
      quad ? DivUp(sa.ye - sa.ys, quad_rpb)
           : std::max<uint32_t>(1, DivUp(sa.box_pixels, h->select_passes == 3 ? kChunk
                                                                              : kSpChunk));
  const uint32_t chunk_slots = quad ? kQuadChunk : kSpChunk;
  uint64_t* d_total = reinterpret_cast<uint64_t*>(s->d_small);
  // the count the host reads: SelScan also stores it in the mapped buffer
  uint64_t* m_total = static_cast<uint64_t*>(MappedResult(s, kMappedSelTotal));
  const double sel_bytes = double(sa.box_pixels) * 4.0 * p->n_images;
  // positions of up to the whole box (single pass) or the counts (three
  // kernels: RDL_SUBMINOR_SELECT=3, for comparison)
  uint32_t* counts = nullptr;
  uint32_t* sel_failed = nullptr;  // single pass: set by a timed-out look-back
  if (h->select_passes == 0) {
    // counts (then offsets), the chunks' local lists, the placed positions
    const size_t slots = size_t(n_chunks) * chunk_slots;
    RDL_TRY(Grow(&h->counts, &h->counts_bytes, size_t(n_chunks) * sizeof(uint32_t) + 64, st));
    RDL_TRY(Grow(&h->local_buf, &h->local_bytes, slots * sizeof(uint32_t), st));
    RDL_TRY(Grow(&h->pos_buf, &h->pos_bytes,
                 std::max<size_t>(sa.box_pixels, 1) * sizeof(uint32_t), st));
    counts = static_cast<uint32_t*>(h->counts);
    ScopedTiming t(s, "subminor_select", sel_bytes);
    if (quad)
      SelLocalQuad<<<n_chunks, kSpThreads, 0, st>>>(sa, quad_ipr, quad_rpb, counts,
                                                    static_cast<uint32_t*>(h->local_buf));
    else
      SelLocal<<<n_chunks, kSpThreads, 0, st>>>(sa, counts,
                                                static_cast<uint32_t*>(h->local_buf));
    SelScan<<<1, 1024, 0, st>>>(counts, n_chunks, d_total, m_total);
    SelPlace<<<n_chunks, 256, 0, st>>>(counts, n_chunks, d_total,
                                       static_cast<const uint32_t*>(h->local_buf), chunk_slots,
                                       static_cast<uint32_t*>(h->pos_buf));
  } else if (h->select_passes == 1) {
    RDL_TRY(Grow(&h->counts, &h->counts_bytes, size_t(n_chunks) * sizeof(uint64_t) + 64, st));
    RDL_TRY(Grow(&h->pos_buf, &h->pos_bytes,
                 std::max<size_t>(sa.box_pixels, 1) * sizeof(uint32_t), st));
    uint64_t* status = static_cast<uint64_t*>(h->counts);
    uint32_t* ticket = reinterpret_cast<uint32_t*>(status + n_chunks);
    sel_failed = ticket + 1;
    RDL_HIP_CHECK(hipMemsetAsync(status, 0, size_t(n_chunks) * sizeof(uint64_t) + 64, st));
    ScopedTiming t(s, "subminor_select", sel_bytes);
    SelSinglePass<<<n_chunks, kSpThreads, 0, st>>>(
        sa, h->select_ticket ? ticket : nullptr, status, n_chunks,
        static_cast<uint32_t*>(h->pos_buf), d_total, sel_failed, h->select_spin_limit);
  } else {
    RDL_TRY(Grow(&h->counts, &h->counts_bytes, size_t(n_chunks) * sizeof(uint32_t) + 64, st));
    counts = static_cast<uint32_t*>(h->counts);
    ScopedTiming t(s, "subminor_select", 2.0 * sel_bytes);
    SelCount<<<n_chunks, kSelThreads, 0, st>>>(sa, counts);
    SelScan<<<1, 1024, 0, st>>>(counts, n_chunks, d_total, m_total);
  }
  RDL_HIP_CHECK(hipGetLastError());
  uint64_t n_sel = 0;
  uint32_t failed = 0;
  {
    // RDL_SEL_COUNT_COPY=1: read the count back by a copy (r04 form; bisect)
    static const bool count_copy = [] {
      const char* e = std::getenv("RDL_SEL_COUNT_COPY");
      return e && e[0] == '1';
    }();
    const SmallRead r[2] = {{&n_sel, h->select_passes == 1 || count_copy ? d_total : m_total,
                             sizeof(n_sel)},
                            {&failed, sel_failed, sizeof(failed)}};
    RDL_TRY(ReadSmall(s, r, sel_failed ? 2 : 1));
  }
  if (failed) {
    SetError("rdl_subminor_run: selection look-back timed out");
    return RDL_ERR_TIMEOUT;
  }
  h->n_selected = n_sel;
  *n_sel_out = n_sel;
  if (n_sel == 0) return RDL_OK;  // subminor_loop.cc:52-54
  const uint32_t ni = p->n_images;
  if (h->select_passes != 3) {
    RDL_TRY(Grow(&h->sel, &h->sel_bytes, 2 * n_sel * ni * sizeof(float) + 256, st));
    h->d_pos = static_cast<uint32_t*>(h->pos_buf);
    h->d_r = static_cast<float*>(h->sel);
    h->d_m = h->d_r + n_sel * ni;
    ScopedTiming t(s, "subminor_select", 12.0 * n_sel * ni);
    const unsigned grid = unsigned(std::min<uint64_t>(DivUp(n_sel, 256), 4096));
    SelGather<<<grid, 256, 0, st>>>(d_residuals, p->width, p->width * p->height, h->d_pos,
                                    n_sel, ni, h->d_r);
  } else {
    const size_t sel_need = n_sel * sizeof(uint32_t) + 2 * n_sel * ni * sizeof(float) + 256;
    RDL_TRY(Grow(&h->sel, &h->sel_bytes, sel_need, st));
    h->d_pos = static_cast<uint32_t*>(h->sel);
    h->d_r = reinterpret_cast<float*>(static_cast<char*>(h->sel) +
                                      (n_sel * sizeof(uint32_t) + 15) / 16 * 16);
    h->d_m = h->d_r + n_sel * ni;
    ScopedTiming t(s, "subminor_select", sel_bytes + 8.0 * n_sel * ni);
    SelScatter<<<n_chunks, kSelThreads, 0, st>>>(sa, counts, ni, n_sel, h->d_pos, h->d_r);
  }
  RDL_HIP_CHECK(hipGetLastError());
  return RDL_OK;
}

}  // namespace rdl
