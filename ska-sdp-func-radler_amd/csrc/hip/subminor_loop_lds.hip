// SubminorLoop: the sub-minor loop with the selection in LDS (global scratch
// when it outgrows the workgroups' LDS). Any number of images, and the only
// loop that runs the log-polynomial fit; the register and table loops take
// every shape they can hold (PlanSubminorLoop, subminor_plan.h).
//
// The selected set is partitioned over G workgroups; each keeps its pixels'
// positions, residual and model values in LDS. Per iteration every workgroup
// subtracts the current component's shifted twice-convolved PSF from its
// pixels (one FMA per pixel and image, PSF gathered from HBM/L2),
// re-integrates and reduces its argmax; with G > 1 the winners are exchanged
// through write-through (sc1) records and a monotonic arrival counter, so all
// workgroups take the same next component.
// From subminor_loop_shared.h: WriteTrace and WriteResult.
#include "subminor_loop_shared.h"

namespace rdl {

// Winner record layout (u32 words): key lo, key hi, integ (f32), pos, r[n_img]
template <int NI>
__global__ __launch_bounds__(kLoopThreads) void SubminorLoop(LoopArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
  __shared__ uint64_t red[kLoopThreads / 64];
  __shared__ uint32_t win[4 + RDL_MAX_IMAGES];
  __shared__ uint32_t flags[2];

  const uint32_t tid = threadIdx.x;
  const uint64_t base = uint64_t(blockIdx.x) * a.per_block;
  const uint32_t cnt =
      base >= a.n_sel ? 0u : uint32_t(min<uint64_t>(a.per_block, a.n_sel - base));
  const uint32_t n_img = a.n_img;

  uint32_t* pos;
  float* R;
  float* M;
  size_t stride;  // between images
  if (a.use_lds) {
    pos = smem;
    R = reinterpret_cast<float*>(smem + a.per_block);
    M = R + size_t(n_img) * a.per_block;
    stride = a.per_block;
    for (uint32_t j = tid; j < cnt; j += kLoopThreads) {
      pos[j] = a.pos[base + j];
      for (uint32_t k = 0; k < n_img; ++k) {
        R[k * stride + j] = a.r[size_t(k) * a.n_sel + base + j];
        M[k * stride + j] = 0.0f;
      }
    }
  } else {
    pos = const_cast<uint32_t*>(a.pos) + base;
    R = a.r + base;
    M = a.m + base;
    stride = a.n_sel;
    for (uint32_t j = tid; j < cnt; j += kLoopThreads)
      for (uint32_t k = 0; k < n_img; ++k) M[k * stride + j] = 0.0f;
  }
  __syncthreads();

  const int W = int(a.width), H = int(a.height);
  const size_t plane = size_t(a.width) * a.height;
  float c[NI];
#pragma unroll
  for (int k = 0; k < NI; ++k) c[k] = 0.0f;
  int cx = 0, cy = 0;
  bool have_component = false;
  float start_abs = 0.0f;
  bool diverging = false;
  float flux = 0.0f;
  uint64_t iteration = a.iteration_start;
  uint32_t gen = 0;
  float m = 0.0f;
  uint64_t winner_p = 0;

  while (true) {
    // ---- subtract the current component, integrate, local argmax
    uint64_t best = 0;
    for (uint32_t j = tid; j < cnt; j += kLoopThreads) {
      const uint32_t pk = pos[j];
      const int px = int(pk & 0xffffu), py = int(pk >> 16);
      float v[NI];
      if (have_component) {
        const int dx = px - cx + W / 2, dy = py - cy + H / 2;
        const bool in = dx >= 0 && dx < W && dy >= 0 && dy < H;
        const size_t off = size_t(dy) * a.width + size_t(dx);
#pragma unroll
        for (int k = 0; k < NI; ++k) {
          if (k < int(n_img)) {
            float rv = R[k * stride + j];
            if (in) {
              const float pv = a.psfs[size_t(k / int(a.n_pol)) * plane + off];
              rv = __builtin_fmaf(-pv, c[k], rv);
              R[k * stride + j] = rv;
            }
            v[k] = rv;
          } else {
            v[k] = 0.0f;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < NI; ++k)
          v[k] = k < int(n_img) ? R[k * stride + j] : 0.0f;
      }
      float integ = IntegratePixel(a.integ, [&](uint32_t kk) {
        float r = v[0];
#pragma unroll
        for (int q = 1; q < NI; ++q) r = (uint32_t(q) == kk) ? v[q] : r;
        return r;
      });
      if (a.rms) integ *= a.rms[size_t(py) * a.width + px];  // GetMaxComponent
      uint64_t key = MaxKey(integ, a.allow_negative, base + j);
      if (base + j == 0 && integ != integ) key = ~0ull;  // scratch[0] is NaN
      best = key > best ? key : best;
    }
    // block reduce
    {
      uint64_t w = WaveMaxU64(best);
      if ((tid & 63) == 0) red[tid >> 6] = w;
      __syncthreads();
      if (tid < 64) {
        uint64_t x = tid < kLoopThreads / 64 ? red[tid] : 0ull;
        x = WaveMaxU64(x);
        if (tid == 0) red[0] = x;
      }
      __syncthreads();
    }
    const uint64_t block_best = red[0];
    // owner of the block winner fills the local record
    if (cnt > 0) {
      const uint64_t lp = block_best == 0 ? 0ull
                          : block_best == ~0ull ? 0ull
                          : uint64_t(0xffffffffu - uint32_t(block_best));
      const uint64_t j = lp - base;
      if (lp >= base && j < cnt && (j % kLoopThreads) == tid) {
        win[0] = uint32_t(block_best);
        win[1] = uint32_t(block_best >> 32);
        float vv[NI];
#pragma unroll
        for (int k = 0; k < NI; ++k)
          vv[k] = k < int(n_img) ? R[k * stride + j] : 0.0f;
        float integ = IntegratePixel(a.integ, [&](uint32_t kk) {
          float r = vv[0];
#pragma unroll
          for (int q = 1; q < NI; ++q) r = (uint32_t(q) == kk) ? vv[q] : r;
          return r;
        });
        if (a.rms)
          integ *= a.rms[size_t(pos[j] >> 16) * a.width + (pos[j] & 0xffffu)];
        win[2] = __float_as_uint(integ);
        win[3] = pos[j];
        for (uint32_t k = 0; k < n_img; ++k) win[4 + k] = __float_as_uint(vv[k]);
      }
    } else if (tid == 0) {
      win[0] = 0;
      win[1] = 0;
    }
    __syncthreads();

    if (a.n_blocks > 1) {
      // ---- exchange records: write-through stores, arrival counter
      uint32_t* rec_base = a.records + size_t(gen & 1) * a.n_blocks * a.rec_words;
      if (tid == 0) {
        uint32_t* rec = rec_base + size_t(blockIdx.x) * a.rec_words;
        for (uint32_t w = 0; w < 4 + n_img; ++w) StoreSc1(rec + w, win[w]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t target = (gen + 1) * a.n_blocks;
        uint64_t spins = 0;
        flags[0] = 0;
        while (LoadSc1(a.counter) < target) {
          __builtin_amdgcn_s_sleep(1);
          if (++spins > (1ull << 28)) {  // ~minutes: a lost workgroup
            flags[0] = 1;
            break;
          }
        }
      }
      __syncthreads();
      if (flags[0]) {
        if (tid == 0) StoreSc1(&a.result[8], 1u);
        return;
      }
      // wave 0 reduces the G keys
      if (tid < 64) {
        uint64_t bk = 0;
        uint32_t bb = 0;
        for (uint32_t b = tid; b < a.n_blocks; b += 64) {
          uint32_t* rec = rec_base + size_t(b) * a.rec_words;
          const uint64_t k =
              uint64_t(LoadSc1(rec)) | (uint64_t(LoadSc1(rec + 1)) << 32);
          if (k > bk) {
            bk = k;
            bb = b;
          }
        }
        // wave argmax over (key, block)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const uint64_t ok = __shfl_xor(bk, off, 64);
          const uint32_t ob = __shfl_xor(bb, off, 64);
          if (ok > bk || (ok == bk && ob < bb)) {
            bk = ok;
            bb = ob;
          }
        }
        if (tid == 0) flags[1] = bb;
      }
      __syncthreads();
      if (tid < 4 + n_img) {
        uint32_t* rec = rec_base + size_t(flags[1]) * a.rec_words;
        win[tid] = LoadSc1(rec + tid);
      }
      __syncthreads();
      ++gen;
    }

    // ---- the global winner is in win[]; identical decisions everywhere
    const uint64_t gkey = uint64_t(win[0]) | (uint64_t(win[1]) << 32);
    winner_p = (gkey == 0 || gkey == ~0ull)
                   ? 0ull
                   : uint64_t(0xffffffffu - uint32_t(gkey));
    m = __uint_as_float(win[2]);
    if (!have_component) {
      start_abs = fabsf(m);  // subminor_loop.cc:59
    } else {
      if (a.divergence_limit != 0.0f)
        diverging = fabsf(m) > start_abs * a.divergence_limit;
      ++iteration;
    }
    // loop condition (subminor_loop.cc:61-63)
    const bool go = fabsf(m) > a.threshold && iteration < a.max_iterations &&
                    (!a.stop_on_negative || m >= 0.0f) && !diverging;
    if (!go) break;
    // next component (subminor_loop.cc:64-89)
    if (a.has_lp) {
      // PerformSpectralFit of the gain-scaled values (subminor_loop.cc:66-76)
      // with the log-polynomial fitter: every thread runs the same fit on
      // the same values (identical bits, no broadcast needed)
      float v[NI];
      for (int k = 0; k < NI; ++k)
        v[k] = k < int(n_img) ? __uint_as_float(win[4 + k]) * a.gain : 0.0f;
      if (a.has_forced) {
        // forced terms of the winner's pixel: one address for the whole
        // workgroup, so the loads and the fit stay wave-uniform
        float terms[lp::kMaxTerms];
        const uint32_t wx = win[3] & 0xffffu, wy = win[3] >> 16;
        for (int k = 0; k < lp::kMaxTerms; ++k) terms[k] = 0.0f;
        if (wx < a.width && wy < a.height)  // (the planes cover the image: checked at launch)
          lp::LoadForcedTerms(a.forced, a.lp.n_terms, wx, wy, terms);
        lp::PerformForcedFit(a.lp, a.forced.weights, terms, a.n_pol, v);
      } else {
        lp::PerformSpectralFit(a.lp, a.n_pol, v);
      }
#pragma unroll
      for (int k = 0; k < NI; ++k) c[k] = k < int(n_img) ? v[k] : 0.0f;
    } else if (a.spectral) {
      // PerformSpectralFit of the gain-scaled values (subminor_loop.cc:66-76)
#pragma unroll
      for (int k = 0; k < NI; ++k) {
        float acc = 0.0f;
        if (k < int(n_img))
          for (uint32_t q = 0; q < n_img; ++q)
            acc = __builtin_fmaf(a.spectral[k * n_img + q],
                                 __uint_as_float(win[4 + q]) * a.gain, acc);
        c[k] = acc;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NI; ++k)
        c[k] = k < int(n_img) ? __uint_as_float(win[4 + k]) * a.gain : 0.0f;
    }
    flux += m * a.gain;
    cx = int(win[3] & 0xffffu);
    cy = int(win[3] >> 16);
    {
      const uint64_t j = winner_p - base;
      if (winner_p >= base && j < cnt && (j % kLoopThreads) == tid) {
#pragma unroll
        for (int k = 0; k < NI; ++k)
          if (k < int(n_img)) M[k * stride + j] += c[k];
      }
    }
    if (blockIdx.x == 0 && tid == 0 && a.trace)
      WriteTrace(a.trace, a.trace_cap, iteration - a.iteration_start, uint32_t(cx),
                 uint32_t(cy));
    have_component = true;
    __syncthreads();
  }

  // write back model values (LDS variant)
  if (a.use_lds) {
    for (uint32_t j = tid; j < cnt; j += kLoopThreads)
      for (uint32_t k = 0; k < n_img; ++k)
        a.m[size_t(k) * a.n_sel + base + j] = M[k * stride + j];
  }
  if (blockIdx.x == 0 && tid == 0) WriteResult(a.result, iteration, m, diverging, flux);
}

template <int NI>
int LaunchLoop(const LoopArgs& a, size_t lds_bytes, hipStream_t stream) {
  auto kernel = SubminorLoop<NI>;
  if (lds_bytes > 0)
    RDL_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes)));
  return LaunchLoopKernel(kernel, a.n_blocks, kLoopThreads, lds_bytes, a, stream);
}

int LaunchLdsLoop(const LoopArgs& a, const LoopPlan& plan, hipStream_t stream) {
  const uint32_t ni = a.n_img;
  if (ni == 1) return LaunchLoop<1>(a, plan.lds_bytes, stream);
  if (ni <= 2) return LaunchLoop<2>(a, plan.lds_bytes, stream);
  if (ni <= 4) return LaunchLoop<4>(a, plan.lds_bytes, stream);
  if (ni <= 8) return LaunchLoop<8>(a, plan.lds_bytes, stream);
  if (ni <= 16) return LaunchLoop<16>(a, plan.lds_bytes, stream);
  return LaunchLoop<RDL_MAX_IMAGES>(a, plan.lds_bytes, stream);
}

}  // namespace rdl
