// The Högbom loop over a stack of independent planes: rdl_hogbom_batch_run.
//
// A batch item is one single-image clean (n_images = 1, the identity
// integration, no fit, no RMS image). rdl_hogbom_run spends two launches per
// component and fills a few CUs with a small plane; here one workgroup owns
// one plane and runs its whole loop, so the device holds as many planes at
// once as it has workgroup slots and a component costs no launch and no host
// round trip. Per plane the bits are those of rdl_find_peak followed by
// rdl_hogbom_run (clean.hip): the argmax key is order-independent
// (rdl::PeakKey), the subtraction is the same fmaf(-psf, f, r), and the
// decisions are HogbomPrepare's and HogbomStep's, statement for statement.
//
// No workgroup waits for another: the only synchronisation is the workgroup
// barrier. A launch runs at most `chunk` components per plane and returns;
// everything a plane needs to go on is in its BatchPlane in device memory, so
// the host relaunches the planes not done and no bit depends on the chunk.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "hogbom_shared.h"
#include "rdl_internal.h"

namespace rdl {

// One active plane's loop, resident in device memory between launches.
struct BatchPlane {
  HogbomState st;           // factors[0]: the pending component's factor
  uint64_t max_iterations;
  float threshold;          // the caller's; first_threshold once started
  float initial_max;
  uint32_t plane;           // index into the stacks
  int32_t started;          // the start peak has been searched
  PeakOut start;            // rdl_find_peak's answer
};

struct BatchArgs {
  float* residuals;
  float* models;
  const float* psfs;
  const uint8_t* mask;
  size_t residual_stride, model_stride, psf_stride, mask_stride;
  BatchPlane* planes;
  const uint32_t* todo;  // the entries of `planes` this launch runs
  uint32_t* done;        // per entry of `planes`
  uint32_t* trace;       // trace_cap pairs per entry, or nullptr
  uint64_t trace_cap;
  uint64_t chunk;
  uint32_t width, height;
  uint32_t bx0, bx1, by0, by1;  // peak-finder border box
  float gain, one_minus_mgain, divergence_limit;
  int32_t allow_negative, stop_on_negative;
  uint32_t flags;
};

// One sweep of the workgroup over rows [y_begin, y_end): inside the window
// the component is subtracted (HogbomPass<1>'s statement), inside the box
// and the mask the pixel enters the argmax. Pixels in neither are not read.
// The threads walk the rows as one flat range, so a plane narrower than the
// workgroup still uses every lane.
__device__ __forceinline__ uint64_t Sweep(const BatchArgs& a, float* residual,
                                          const float* psf, const uint8_t* mask,
                                          const Window& w, float f, uint32_t y_begin,
                                          uint32_t y_end) {
  uint64_t best = 0;
  const uint32_t width = a.width;
  const uint32_t step_y = blockDim.x / width, step_x = blockDim.x % width;
  uint32_t y = y_begin + threadIdx.x / width, x = threadIdx.x % width;
  while (y < y_end) {
    const bool in_w = y >= w.y0 && y < w.y1 && x >= w.x0 && x < w.x1;
    const bool in_b = y >= a.by0 && y < a.by1 && x >= a.bx0 && x < a.bx1;
    if (in_w || in_b) {
      const uint32_t idx = y * width + x;
      float r = residual[idx];
      if (in_w) {
        const float pv = psf[size_t(int64_t(y) - w.off_y) * width +
                             size_t(int64_t(x) - w.off_x)];
        r = __builtin_fmaf(-pv, f, r);
        residual[idx] = r;
      }
      if (in_b && (!mask || mask[idx])) {
        const uint64_t k = PeakKey(r, a.allow_negative, idx);
        best = k > best ? k : best;
      }
    }
    x += step_x;
    y += step_y;
    if (x >= width) {
      x -= width;
      y += 1;
    }
  }
  return best;
}

// HogbomPrepare (clean.hip) for one image without a fit: the stop test and,
// if the loop goes on, the factor, the model update and the trace entry.
__device__ void BatchPrepare(const BatchArgs& a, BatchPlane& bp, const float* residual,
                             float* model, uint32_t* trace) {
  HogbomState& st = bp.st;
  const float m = st.peak_value;
  const bool go = st.found && fabsf(m) > bp.threshold &&
                  st.iteration < bp.max_iterations &&
                  !(m < 0.0f && a.stop_on_negative) && !st.diverging;
  if (!go) {
    st.done = 1;
    return;
  }
  const uint32_t idx = st.peak_index;
  float v = residual[idx];
  v *= a.gain;
  st.factors[0] = v;
  model[idx] += v;
  const uint64_t t = st.iteration - st.first_iteration;
  if (trace && t < a.trace_cap) {
    trace[2 * t] = idx % a.width;
    trace[2 * t + 1] = idx / a.width;
  }
}

template <int kThreads>
__global__ __launch_bounds__(kThreads) void HogbomBatch(BatchArgs a) {
  __shared__ uint64_t lds[16];
  // the pending component, published by thread 0 between two barriers
  __shared__ uint32_t sh_done, sh_index;
  __shared__ float sh_factor;
  const uint32_t entry = a.todo[blockIdx.x];
  BatchPlane& bp = a.planes[entry];
  HogbomState& st = bp.st;
  const size_t b = bp.plane;
  float* residual = a.residuals + b * a.residual_stride;
  float* model = a.models + b * a.model_stride;
  const float* psf = a.psfs + b * a.psf_stride;
  const uint8_t* mask = a.mask ? a.mask + b * a.mask_stride : nullptr;
  uint32_t* trace = a.trace ? a.trace + size_t(entry) * 2 * a.trace_cap : nullptr;
  const bool box = a.bx1 > a.bx0 && a.by1 > a.by0;

  // every thread reads `started` before the first barrier below; thread 0
  // writes it after that barrier
  if (!bp.started) {
    if (a.flags & RDL_HOGBOM_BATCH_LOAD_RULE) {
      // ImageSet::LoadAndAverage for one entry of weight 1: fmaf(x, 1, +0)
      // and a scale by 1 change -0 to +0 and nothing else
      const uint32_t n = a.width * a.height;
      for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        if (__float_as_uint(residual[i]) == 0x80000000u) residual[i] = 0.0f;
        if (__float_as_uint(model[i]) == 0x80000000u) model[i] = 0.0f;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    // rdl_find_peak: the box alone, nothing to subtract
    const Window none{0, 0, 0, 0, 0, 0};
    uint64_t best = box ? Sweep(a, residual, psf, mask, none, 0.0f, a.by0, a.by1) : 0ull;
    best = BlockMaxU64(best, lds);
    if (threadIdx.x == 0) {
      PeakOut o;
      PeakOutOfKey(best, residual, a.width, a.height, 1, mask != nullptr, &o);
      bp.start = o;
      // generic_clean.cc:138-142 with MajorIterationThreshold() = 0
      bp.initial_max = fabsf(o.value);
      const float by_gain = bp.initial_max * a.one_minus_mgain;
      const float major_iter_threshold = 0.0f < by_gain ? by_gain : 0.0f;  // std::max(0, .)
      if (major_iter_threshold > bp.threshold) bp.threshold = major_iter_threshold;
      st.peak_index = o.y * a.width + o.x;
      st.peak_value = o.value;
      st.found = o.found;
      bp.started = 1;
      BatchPrepare(a, bp, residual, model, trace);
    }
  }
  if (threadIdx.x == 0) {
    sh_done = st.done;
    sh_index = st.peak_index;
    sh_factor = st.factors[0];
  }
  __syncthreads();

  for (uint64_t it = 0; it < a.chunk; ++it) {
    if (sh_done) break;  // the same for every thread
    const uint32_t index = sh_index;
    const float f = sh_factor;
    const Window w = SubtractWindow(a.width, a.height, index % a.width, index / a.width);
    // the rows of the window and of the box, as one range (rows between the
    // two, when they are apart, are skipped pixel by pixel)
    const bool win = w.x1 > w.x0 && w.y1 > w.y0;
    uint32_t y_begin = 0, y_end = 0;
    if (win && box) {
      y_begin = min(w.y0, a.by0);
      y_end = max(w.y1, a.by1);
    } else if (win) {
      y_begin = w.y0;
      y_end = w.y1;
    } else if (box) {
      y_begin = a.by0;
      y_end = a.by1;
    }
    uint64_t best = Sweep(a, residual, psf, mask, w, f, y_begin, y_end);
    // The winner's pixel was stored by whichever thread swept it and is read
    // back by thread 0: every wave's stores have left it before it joins the
    // barrier, and the workgroup's waves share one CU and its L1.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    best = BlockMaxU64(best, lds);  // its first barrier also ends the reads of sh_*
    if (threadIdx.x == 0) {
      // HogbomStep (clean.hip), FindPeak -> Find / FindWithMask
      if (best != 0) {
        st.peak_index = 0xffffffffu - uint32_t(best & 0xffffffffu);
        st.found = 1;
      } else if (!mask) {
        st.peak_index = 0;  // Avx<>: no qualifying pixel -> index 0
        st.found = 1;
      } else {
        st.found = 0;
      }
      if (st.found) st.peak_value = residual[st.peak_index];
      if (st.found && a.divergence_limit != 0.0f)
        st.diverging = fabsf(st.peak_value) > bp.initial_max * a.divergence_limit;
      st.iteration += 1;
      BatchPrepare(a, bp, residual, model, trace);
      sh_done = st.done;
      sh_index = st.peak_index;
      sh_factor = st.factors[0];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) a.done[entry] = st.done;
}

// Components per plane and launch. One workgroup of 1024 threads takes 0.55 ms
// a component on a 1024 x 1024 plane, the largest this entry point takes
// (profiles/hogbom_batch_timing.txt: 200 components in 110 ms), so 2048
// components keep the longest launch around a second.
constexpr uint64_t kDefaultChunk = 2048;

uint64_t BatchChunk() {
  if (const char* e = std::getenv("RDL_HOGBOM_BATCH_CHUNK")) {
    const long long v = std::atoll(e);
    if (v > 0) return uint64_t(v);
  }
  return kDefaultChunk;
}

}  // namespace rdl

extern "C" {

int rdl_hogbom_batch_run(rdl_session* s, const rdl_hogbom_batch_params* p,
                         const float* h_threshold, const uint64_t* h_iteration_start,
                         const uint64_t* h_max_iterations, const uint8_t* h_active,
                         rdl_hogbom_batch_out* h_out, uint32_t* h_trace,
                         uint64_t trace_cap) {
  RDL_ARG_CHECK(s && p && h_threshold && h_iteration_start && h_max_iterations && h_active &&
                    h_out,
                "NULL argument");
  RDL_ARG_CHECK(p->d_residuals && p->d_models && p->d_psfs, "NULL argument");
  RDL_ARG_CHECK(p->n_planes > 0, "no planes");
  RDL_ARG_CHECK((p->flags & ~RDL_HOGBOM_BATCH_LOAD_RULE) == 0, "unknown flag");
  RDL_ARG_CHECK(p->width > 0 && p->height > 0, "empty image");
  const uint64_t n = uint64_t(p->width) * p->height;
  RDL_ARG_CHECK(n <= RDL_HOGBOM_BATCH_MAX_PIXELS,
                "plane above 2^20 pixels: rdl_hogbom_run fills the device with it");
  RDL_ARG_CHECK(p->residual_stride >= n, "residual stride smaller than a plane");
  RDL_ARG_CHECK(p->model_stride >= n, "model stride smaller than a plane");
  RDL_ARG_CHECK(p->psf_stride == 0 || p->psf_stride >= n, "psf stride smaller than a plane");
  RDL_ARG_CHECK(!p->d_mask || p->mask_stride == 0 || p->mask_stride >= n,
                "mask stride smaller than a plane");

  std::vector<rdl::BatchPlane> planes;
  for (uint32_t b = 0; b < p->n_planes; ++b) {
    if (!h_active[b]) continue;
    rdl::BatchPlane bp{};
    bp.st.iteration = h_iteration_start[b];
    bp.st.first_iteration = h_iteration_start[b];
    bp.max_iterations = h_max_iterations[b];
    bp.threshold = h_threshold[b];
    bp.plane = b;
    planes.push_back(bp);
  }
  const size_t n_active = planes.size();
  if (n_active == 0) return RDL_OK;

  rdl::BatchArgs a{};
  a.residuals = p->d_residuals;
  a.models = p->d_models;
  a.psfs = p->d_psfs;
  a.mask = p->d_mask;
  a.residual_stride = p->residual_stride;
  a.model_stride = p->model_stride;
  a.psf_stride = p->psf_stride;
  a.mask_stride = p->d_mask ? p->mask_stride : 0;
  a.width = p->width;
  a.height = p->height;
  a.gain = p->gain;
  a.one_minus_mgain = 1.0f - p->major_loop_gain;
  a.divergence_limit = p->divergence_limit;
  a.allow_negative = p->allow_negative;
  a.stop_on_negative = p->stop_on_negative;
  a.flags = p->flags;
  a.chunk = rdl::BatchChunk();
  // rdl_hogbom_run's box; empty exactly when rdl_find_peak's is
  a.bx0 = p->h_border;
  a.bx1 = p->width - p->h_border;
  if (a.bx1 < a.bx0 || a.bx1 > p->width) a.bx1 = a.bx0;
  a.by0 = p->v_border;
  a.by1 = p->height - p->v_border;
  if (a.by1 < a.by0 || a.by1 > p->height) a.by1 = a.by0;

  // device: planes | todo | done | trace
  const uint64_t n_trace = (h_trace && trace_cap) ? trace_cap : 0;
  const size_t plane_bytes = (n_active * sizeof(rdl::BatchPlane) + 255) / 256 * 256;
  const size_t list_bytes = (n_active * sizeof(uint32_t) + 255) / 256 * 256;
  const size_t trace_bytes = n_active * n_trace * 2 * sizeof(uint32_t);
  RDL_TRY(s->EnsureScratch(s->loop_state, plane_bytes + 2 * list_bytes + trace_bytes));
  char* buf = static_cast<char*>(s->loop_state.ptr);
  a.planes = reinterpret_cast<rdl::BatchPlane*>(buf);
  uint32_t* d_todo = reinterpret_cast<uint32_t*>(buf + plane_bytes);
  a.todo = d_todo;
  a.done = reinterpret_cast<uint32_t*>(buf + plane_bytes + list_bytes);
  a.trace = n_trace ? reinterpret_cast<uint32_t*>(buf + plane_bytes + 2 * list_bytes) : nullptr;
  a.trace_cap = n_trace;
  RDL_HIP_CHECK(rdl::UploadSync(a.planes, planes.data(), n_active * sizeof(rdl::BatchPlane),
                                s->stream));

  // small planes get small workgroups, so that thousands are resident at once
  const int threads = n <= 4096 ? 64 : n <= 65536 ? 256 : 1024;
  std::vector<uint32_t> todo(n_active), done(n_active);
  for (size_t i = 0; i < n_active; ++i) todo[i] = uint32_t(i);
  while (!todo.empty()) {
    const uint32_t grid = uint32_t(todo.size());
    RDL_HIP_CHECK(rdl::UploadSync(d_todo, todo.data(), grid * sizeof(uint32_t), s->stream));
    {
      rdl::ScopedTiming t(s, "hogbom_batch", 0.0);
      if (threads == 64)
        rdl::HogbomBatch<64><<<grid, 64, 0, s->stream>>>(a);
      else if (threads == 256)
        rdl::HogbomBatch<256><<<grid, 256, 0, s->stream>>>(a);
      else
        rdl::HogbomBatch<1024><<<grid, 1024, 0, s->stream>>>(a);
    }
    RDL_HIP_CHECK(hipGetLastError());
    // the done flags, 64 KiB of them at a time
    const size_t piece = (size_t(1) << 16) / sizeof(uint32_t);
    for (size_t i = 0; i < n_active; i += piece) {
      const size_t m = std::min(piece, n_active - i);
      const rdl::SmallRead r{done.data() + i, a.done + i, m * sizeof(uint32_t)};
      RDL_TRY(rdl::ReadSmall(s, &r, 1));
    }
    std::vector<uint32_t> next;
    for (uint32_t e : todo)
      if (!done[e]) next.push_back(e);
    todo.swap(next);
  }

  RDL_HIP_CHECK(hipMemcpyAsync(planes.data(), a.planes, n_active * sizeof(rdl::BatchPlane),
                               hipMemcpyDeviceToHost, s->stream));
  std::vector<uint32_t> trace(n_active * n_trace * 2);
  if (n_trace)
    RDL_HIP_CHECK(hipMemcpyAsync(trace.data(), a.trace, trace_bytes, hipMemcpyDeviceToHost,
                                 s->stream));
  RDL_HIP_CHECK(hipStreamSynchronize(s->stream));
  for (size_t i = 0; i < n_active; ++i) {
    const rdl::BatchPlane& bp = planes[i];
    rdl_hogbom_batch_out& o = h_out[bp.plane];
    o.result.iteration = bp.st.iteration;
    o.result.found = bp.st.found;
    o.result.peak = bp.st.peak_value;
    o.result.x = bp.st.peak_index % p->width;
    o.result.y = bp.st.peak_index / p->width;
    o.result.diverging = bp.st.diverging;
    o.start.value = bp.start.value;
    o.start.x = bp.start.x;
    o.start.y = bp.start.y;
    o.start.found = bp.start.found;
    o.first_threshold = bp.threshold;
    if (n_trace) {
      const uint64_t k = std::min<uint64_t>(bp.st.iteration - bp.st.first_iteration, n_trace);
      std::memcpy(h_trace + size_t(bp.plane) * 2 * trace_cap, trace.data() + i * n_trace * 2,
                  k * 2 * sizeof(uint32_t));
    }
  }
  return RDL_OK;
}

}  // extern "C"
