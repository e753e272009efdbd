// The sub-minor (Clark-style) loop: replaces SubMinorLoop::Run with
// findPeakPositions / MakeSets / GetMaxComponent
// (cpp/algorithms/subminor_loop.cc:13-184).
//
// Selection (subminor_select.hip): the sparse two-phase selection. Every
// chunk of the border box flags its pixels once and stores its count and its
// selected positions in its own slot; a scan turns the counts into offsets
// and the non-empty chunks move their positions there. The list is row-major
// (packed y<<16|x), the order the reference's nested x/y loops produce; the
// pixels' N_img residual values are gathered once the host knows the count.
//
// Loop: one persistent launch of the kernel PlanSubminorLoop
// (subminor_plan.h) chooses. By default a selection gets a pairwise PSF
// table, so an iteration reads one contiguous row per PSF instead of
// gathering from the PSF plane, and each thread keeps its pixels' positions,
// residual and model values in registers: SubminorLoopTab (one image) and
// SubminorLoopTabN (joined images) in subminor_loop_tab.hip, SubminorLoopReg
// for every other shape of up to 8 images in subminor_loop_reg.hip. The
// LDS-resident SubminorLoop (subminor_loop_lds.hip) takes more images and the
// log-polynomial fit. Per iteration every workgroup subtracts the current
// component's shifted twice-convolved PSF from its pixels, re-integrates and
// reduces its argmax; with G > 1 workgroups the winners are exchanged through
// write-through records, so all workgroups take the same next component. The
// per-iteration argmax key orders the signed (or absolute) integrated value
// with the first index winning ties, which is GetMaxComponent's
// "start at scratch[0], strict '>'" scan.
//
// This file: the handle, and the sequence of one run (SubminorLaunch,
// SubminorCollect). subminor_model.hip uses the finished loop's model values.
#include "subminor_internal.h"

namespace rdl {

int Grow(void** p, size_t* have, size_t need, hipStream_t stream) {
  if (*have >= need) return RDL_OK;
  if (*p) {
    RDL_HIP_CHECK(hipStreamSynchronize(stream));
    RDL_HIP_CHECK(rdl::DevFree(*p));
    *p = nullptr;
    *have = 0;
  }
  RDL_HIP_CHECK(rdl::DevMalloc(p, need));
  *have = need;
  // RDL_POISON=1: NaN bytes in every fresh buffer (uninitialised reads show)
  if (PoisonOn()) RDL_HIP_CHECK(hipMemsetAsync(*p, 0xff, need, stream));
  return RDL_OK;
}

namespace {

void EnvU32(const char* name, uint32_t* v) {
  if (const char* e = std::getenv(name)) *v = uint32_t(std::strtoul(e, nullptr, 10));
}

SubminorTuning TuningFromEnv() {
  SubminorTuning t;
  // experiments: RDL_SUBMINOR_WAVE_MAX=0 disables the single-wave kernel
  EnvU32("RDL_SUBMINOR_WAVE_MAX", &t.wave_max);
  EnvU32("RDL_SUBMINOR_BIG_MAX", &t.big_max);
  EnvU32("RDL_SUBMINOR_TARGET", &t.target_per_block);  // pixels x images per workgroup
  EnvU32("RDL_SUBMINOR_BIG_TARGET", &t.big_target);
  if (const char* e = std::getenv("RDL_SUBMINOR_TAB")) t.tab = std::atoi(e);
  EnvU32("RDL_SUBMINOR_TAB_TARGET", &t.tab_target);
  if (const char* e = std::getenv("RDL_SUBMINOR_TAB_SINGLE"))
    t.tab_single = uint32_t(std::min<unsigned long>(std::strtoul(e, nullptr, 10), 16384));
  EnvU32("RDL_SUBMINOR_TAB_THREADS", &t.tab_threads);
  // RDL_SUBMINOR_TABLE_MAX=0 keeps the per-iteration PSF gathers
  EnvU32("RDL_SUBMINOR_TABLE_MAX", &t.table_max);
  return t;
}

}  // namespace
}  // namespace rdl

extern "C" {

int rdl_subminor_create(rdl_session* s, rdl_subminor** out) {
  RDL_ARG_CHECK(s && out, "NULL argument");
  auto h = new rdl_subminor();
  h->s = s;
  h->tuning = rdl::TuningFromEnv();
  // RDL_SUBMINOR_SELECT=1 (2): the single-pass look-back selection (chunks
  // in ticket / blockIdx order); 3: count + scan + scatter (comparisons)
  if (const char* e = std::getenv("RDL_SUBMINOR_SELECT")) {
    const int v = std::atoi(e);
    h->select_passes = v == 3 ? 3 : v == 1 || v == 2 ? 1 : 0;
    h->select_ticket = v == 2 ? 0 : 1;
    h->select_quad = v == 4 ? 0 : 1;  // 4: the sparse selection's scalar loads
  }
  // test hook: RDL_SELECT_SPIN_LIMIT=0 makes any look-back wait fail
  if (const char* e = std::getenv("RDL_SELECT_SPIN_LIMIT"))
    h->select_spin_limit = std::strtoull(e, nullptr, 10);
  *out = h;
  return RDL_OK;
}

int rdl_subminor_destroy(rdl_subminor* h) {
  if (!h) return RDL_OK;
  if (rdl::ShutDown()) return RDL_OK;  // rdl_shutdown released everything
  if (h->s->loop_owner == h) h->s->loop_owner = nullptr;
  (void)hipStreamSynchronize(h->s->stream);
  if (h->counts) (void)rdl::DevFree(h->counts);
  if (h->sel) (void)rdl::DevFree(h->sel);
  if (h->pos_buf) (void)rdl::DevFree(h->pos_buf);
  if (h->local_buf) (void)rdl::DevFree(h->local_buf);
  if (h->stamp_mark) (void)rdl::DevFree(h->stamp_mark);
  if (h->sync) (void)rdl::DevFree(h->sync);
  if (h->table) (void)rdl::DevFree(h->table);
  delete h;
  return RDL_OK;
}

int rdl_subminor_set_tuning(rdl_subminor* h, int mode,
                            uint32_t target_per_block) {
  RDL_ARG_CHECK(h, "NULL argument");
  RDL_ARG_CHECK(mode >= 0 && mode <= 6, "mode must be 0 to 6");
  h->tuning.mode = mode;
  if (mode == 6) {  // the table kernel: target_per_block = pixels per participant
    if (target_per_block) h->tuning.tab_target = target_per_block;
    return RDL_OK;
  }
  if (target_per_block) h->tuning.target_per_block = target_per_block;
  return RDL_OK;
}

namespace {
int SubminorLaunch(rdl_subminor* h, const float* d_residuals, const float* d_psfs,
                   const rdl_subminor_params* p, rdl_subminor_result* out, uint64_t trace_cap,
                   uint32_t** trace_dev);
int SubminorCollect(rdl_subminor* h, rdl_subminor_result* out, uint32_t* h_trace,
                    uint64_t trace_cap, const uint32_t* trace_dev);
}  // namespace

int rdl_subminor_run(rdl_subminor* h, const float* d_residuals,
                     const float* d_psfs, const rdl_subminor_params* p,
                     rdl_subminor_result* out, uint32_t* h_trace,
                     uint64_t trace_cap) {
  RDL_ARG_CHECK(h && d_residuals && d_psfs && p && out, "NULL argument");
  RDL_ARG_CHECK(!h->pending, "rdl_subminor_run: the previous loop was not collected");
  uint32_t* trace_dev = nullptr;
  const uint64_t cap = h_trace ? trace_cap : 0;
  RDL_TRY(SubminorLaunch(h, d_residuals, d_psfs, p, out, cap, &trace_dev));
  if (!h->pending) return RDL_OK;  // nothing selected: no loop
  return SubminorCollect(h, out, h_trace, cap, trace_dev);
}

int rdl_subminor_launch(rdl_subminor* h, const float* d_residuals, const float* d_psfs,
                        const rdl_subminor_params* p, rdl_subminor_result* out) {
  RDL_ARG_CHECK(h && d_residuals && d_psfs && p && out, "NULL argument");
  RDL_ARG_CHECK(!h->pending, "rdl_subminor_launch: the previous loop was not collected");
  uint32_t* trace_dev = nullptr;
  return SubminorLaunch(h, d_residuals, d_psfs, p, out, 0, &trace_dev);
}

int rdl_subminor_collect(rdl_subminor* h, rdl_subminor_result* out) {
  RDL_ARG_CHECK(h && out, "NULL argument");
  if (!h->pending) return RDL_OK;  // nothing was launched (no selection)
  return SubminorCollect(h, out, nullptr, 0, nullptr);
}

namespace {

int ValidateParams(const rdl_subminor* h, const rdl_subminor_params* p) {
  RDL_ARG_CHECK(p->n_images >= 1 && p->n_images <= RDL_MAX_IMAGES,
                "n_images out of range");
  RDL_ARG_CHECK(p->n_pol >= 1 && p->n_images % p->n_pol == 0, "bad n_pol");
  RDL_ARG_CHECK(!p->logpoly || (p->logpoly->n_channels * p->n_pol == p->n_images &&
                                p->logpoly->n_channels <= RDL_LOGPOLY_MAX_CHANNELS &&
                                p->logpoly->n_terms >= 1 &&
                                p->logpoly->n_terms <= RDL_LOGPOLY_MAX_TERMS),
                "log-polynomial fit does not match the images");
  const rdl_forced_terms* forced = rdl::lp::ForcedTermsOf(p->logpoly);
  RDL_ARG_CHECK(!forced || rdl::lp::ForcedTermsCover(*forced, p->logpoly->n_terms, p->width,
                                                     p->height),
                "forced-term planes do not cover the image");
  RDL_ARG_CHECK(p->width > 0 && p->height > 0 && p->width <= 65535 &&
                    p->height <= 65535,
                "image size out of range (1..65535)");
  // one mapped result slot per session (kMappedLoop): a second handle's
  // launch would overwrite a result that is still to be collected
  RDL_ARG_CHECK(!h->s->loop_owner || h->s->loop_owner == h,
                "another rdl_subminor handle of this session has a launched loop that was "
                "not collected (rdl_subminor_collect it first)");
  return RDL_OK;
}

// the loop kernels' arguments, but for the exchange area and the table
rdl::LoopArgs MakeLoopArgs(const rdl_subminor* h, const float* d_psfs,
                           const rdl_subminor_params* p, uint64_t n_sel,
                           const rdl::LoopPlan& plan) {
  const bool lpfit = p->logpoly != nullptr;
  rdl::LoopArgs la{};
  la.pos = h->d_pos;
  la.r = h->d_r;
  la.m = h->d_m;
  la.psfs = d_psfs;
  la.n_sel = n_sel;
  la.per_block = uint32_t(plan.per_block);
  la.n_blocks = plan.n_blocks;
  la.rec_words = (4 + p->n_images + 3) / 4 * 4;
  la.width = p->width;
  la.height = p->height;
  la.n_img = p->n_images;
  la.n_pol = p->n_pol;
  la.integ = p->integ;
  la.threshold = p->threshold;
  la.gain = p->gain;
  la.spectral = lpfit ? nullptr : p->d_spectral;
  la.rms = p->d_rms;
  if (lpfit) {
    la.lp = *p->logpoly;
    la.has_lp = 1;
    if (const rdl_forced_terms* forced = rdl::lp::ForcedTermsOf(p->logpoly)) {
      la.forced = *forced;
      la.has_forced = 1;
    }
  }
  la.divergence_limit = p->divergence_limit;
  la.iteration_start = p->iteration_start;
  la.max_iterations = p->max_iterations;
  la.allow_negative = p->allow_negative;
  la.stop_on_negative = p->stop_on_negative;
  la.use_lds = plan.use_lds ? 1 : 0;
  la.prof = h->s->trace_subminor_phases ? 1 : 0;
  la.part_stride = plan.part_stride;
  const char* e = std::getenv("RDL_SUBMINOR_EXCHANGE");  // read per run (tests toggle it)
  la.agent_exchange = e && std::strcmp(e, "agent") == 0 ? 1 : 0;
  const char* at = std::getenv("RDL_SUBMINOR_ATOMIC");  // read per run (A/B in one job)
  la.atomic_reduce = at && at[0] == '0' ? 0 : 1;
  return la;
}

// The per-launch device state: counter, records and trace in h->sync, the
// result in the mapped buffer, and the pairwise table where the plan has one.
int SetUpExchange(rdl_subminor* h, const float* d_psfs, const rdl_subminor_params* p,
                  const rdl::LoopPlan& plan, uint64_t n_trace, rdl::LoopArgs* la) {
  rdl_session* s = h->s;
  hipStream_t st = s->stream;
  const uint64_t n_sel = la->n_sel;
  const size_t rec_bytes = plan.rec_bytes;
  const size_t sync_need = 256 + 256 + rec_bytes + n_trace * 8;
  RDL_TRY(rdl::Grow(&h->sync, &h->sync_bytes, sync_need, st));
  char* sb = static_cast<char*>(h->sync);
  la->counter = reinterpret_cast<uint32_t*>(sb);
  // the result (and the timeout flag, word 8) goes straight to the mapped
  // buffer: no read-back copy; the previous run's words are cleared here (the
  // stream is idle: every run ends in ReadSmall's sync)
  la->result = static_cast<uint32_t*>(rdl::MappedResult(s, rdl::kMappedLoop));
  if (rdl::ZeroCopyOn())
    std::memset(static_cast<char*>(s->m_small) + rdl::kMappedLoop, 0, 256);
  else
    RDL_HIP_CHECK(hipMemsetAsync(la->result, 0, 256, st));
  la->records = reinterpret_cast<uint32_t*>(sb + 512);
  la->trace = n_trace ? reinterpret_cast<uint32_t*>(sb + 512 + rec_bytes) : nullptr;
  la->trace_cap = n_trace;
  // zero counter, result and (every kernel but the LDS one) the epoch-tagged
  // granules: with a pairwise table, by BuildPairTable
  const size_t zero_bytes = plan.kind != rdl::LoopKind::Lds ? 512 + rec_bytes : 512;
  // RDL_TABLE_ZERO=0: a separate memset of the exchange area (r04 form; bisect)
  static const bool table_zero_on = [] {
    const char* e = std::getenv("RDL_TABLE_ZERO");
    return !(e && e[0] == '0');
  }();
  const bool table_zeroes = plan.build_table && table_zero_on;
  if (!table_zeroes) RDL_HIP_CHECK(hipMemsetAsync(sb, 0, zero_bytes, st));
  la->table = nullptr;
  if (plan.build_table) {
    const uint32_t n_psf = p->n_images / p->n_pol;
    // (+ 32 KiB: the table loop reads whole workgroup-sized slices of a row)
    const size_t table_bytes = size_t(n_psf) * n_sel * n_sel * sizeof(float) + (32 << 10);
    RDL_TRY(rdl::Grow(&h->table, &h->table_bytes, table_bytes, st));
    rdl::ScopedTiming t(s, "subminor_table", 8.0 * double(n_psf) * n_sel * n_sel);
    RDL_TRY(rdl::LaunchPairTable(h->d_pos, d_psfs, uint32_t(n_sel), n_psf, p->width, p->height,
                                 static_cast<float*>(h->table), reinterpret_cast<uint64_t*>(sb),
                                 table_zeroes ? uint32_t((zero_bytes + 7) / 8) : 0u, st));
    la->table = static_cast<const float*>(h->table);
  }
  return RDL_OK;
}

int SubminorLaunch(rdl_subminor* h, const float* d_residuals, const float* d_psfs,
                   const rdl_subminor_params* p, rdl_subminor_result* out, uint64_t trace_cap,
                   uint32_t** trace_dev) {
  RDL_ARG_CHECK(h && d_residuals && d_psfs && p && out, "NULL argument");
  RDL_TRY(ValidateParams(h, p));
  rdl_session* s = h->s;
  hipStream_t st = s->stream;
  h->width = p->width;
  h->height = p->height;
  h->n_images = p->n_images;

  // ---------------- selection (subminor_loop.cc:143-184)
  uint64_t n_sel = 0;
  RDL_TRY(rdl::RunSelection(h, d_residuals, p, &n_sel));
  out->n_selected = n_sel;
  out->iteration = p->iteration_start;
  out->diverging = 0;
  out->flux_cleaned = 0.0f;
  if (n_sel == 0) {  // subminor_loop.cc:52-54
    out->has_peak = 0;
    out->peak = 0.0f;
    return RDL_OK;
  }

  // ---------------- partition and loop
  rdl::SubminorShape shape;
  shape.n_sel = n_sel;
  shape.n_images = p->n_images;
  shape.n_pol = p->n_pol;
  shape.integ_mode = p->integ.mode;
  shape.copy_fast_path = p->integ.copy_fast_path != 0;
  shape.has_rms = p->d_rms != nullptr;
  shape.has_spectral = p->d_spectral != nullptr;
  shape.has_logpoly = p->logpoly != nullptr;
  shape.n_cus = s->n_cus;
  shape.coop_limit = s->coop_limit;
  const rdl::LoopPlan plan = rdl::PlanSubminorLoop(h->tuning, shape);
  if (plan.error) {
    rdl::SetError(plan.error_text);
    return plan.error;
  }
  rdl::LoopArgs la = MakeLoopArgs(h, d_psfs, p, n_sel, plan);
  RDL_TRY(SetUpExchange(h, d_psfs, p, plan, trace_cap, &la));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (s->trace_subminor) {
    ev0 = s->GetEvent();
    ev1 = s->GetEvent();
    RDL_HIP_CHECK(hipEventRecord(ev0, st));
  }
  {
    rdl::ScopedTiming t(s, "subminor_loop", 0.0);
    switch (plan.kind) {
      case rdl::LoopKind::Tab:
      case rdl::LoopKind::TabN: RDL_TRY(rdl::LaunchTabLoop(la, plan, st)); break;
      case rdl::LoopKind::Lds: RDL_TRY(rdl::LaunchLdsLoop(la, plan, st)); break;
      default: RDL_TRY(rdl::LaunchRegLoop(la, plan, st)); break;
    }
  }
  if (s->trace_subminor) RDL_HIP_CHECK(hipEventRecord(ev1, st));
  out->has_peak = 1;  // a selection: the loop's first component exists
  h->pending = true;
  s->loop_owner = h;
  h->pending_start = p->iteration_start;
  h->pending_bytes_per_it = 12.0 * double(p->n_images) * double(n_sel);
  h->pending_result = la.result;
  h->pending_ev0 = ev0;
  h->pending_ev1 = ev1;
  h->pending_n_sel = n_sel;
  h->pending_g = plan.n_blocks;
  h->pending_kind = plan.trace_kind;
  h->pending_threads = int(plan.threads);
  h->pending_table = la.table ? 1 : 0;
  *trace_dev = la.trace;
  return RDL_OK;
}

int SubminorCollect(rdl_subminor* h, rdl_subminor_result* out, uint32_t* h_trace,
                    uint64_t trace_cap, const uint32_t* trace_dev) {
  rdl_session* s = h->s;
  hipStream_t st = s->stream;
  h->pending = false;
  if (s->loop_owner == h) s->loop_owner = nullptr;
  rdl::LoopResult res{};
  uint32_t err = 0;
  {
    // the result (words 0-5) and the exchange's timeout flag (word 8) in ONE
    // read: each read-back is a blit launch plus host latency per component run
    static_assert(sizeof(rdl::LoopResult) <= 8 * sizeof(uint32_t), "result before word 8");
    uint32_t raw[9];
    const rdl::SmallRead r{raw, h->pending_result, sizeof(raw)};
    RDL_TRY(rdl::ReadSmall(s, &r, 1));
    std::memcpy(&res, raw, sizeof(res));
    err = raw[8];
  }
  if (err) {
    rdl::SetError("sub-minor loop: grid exchange timed out");
    return RDL_ERR_TIMEOUT;
  }
  // algorithmic bytes: 12 B x N_img x N_sel per iteration
  rdl::AddTimingBytes(s, "subminor_loop",
                      h->pending_bytes_per_it * double(res.iteration - h->pending_start));
  if (s->trace_subminor) {
    const hipEvent_t ev0 = h->pending_ev0, ev1 = h->pending_ev1;
    float ms = 0.0f;
    RDL_HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    {
      const std::lock_guard<std::recursive_mutex> lock(s->timing_mutex);
      s->event_pool.push_back(ev0);
      s->event_pool.push_back(ev1);
    }
    uint64_t ph[6] = {};
    const rdl::SmallRead r{ph, h->pending_result + 16, sizeof(ph)};
    RDL_TRY(rdl::ReadSmall(s, &r, 1));
    std::fprintf(stderr,
                 "[subminor] n_sel=%llu g=%u kind=%d threads=%d table=%d iters=%llu us=%.1f "
                 "gather=%llu integ=%llu wred=%llu bar=%llu xchg=%llu dec=%llu\n",
                 (unsigned long long)h->pending_n_sel, h->pending_g, h->pending_kind,
                 h->pending_threads, h->pending_table,
                 (unsigned long long)(res.iteration - h->pending_start),
                 double(ms) * 1e3, (unsigned long long)ph[0], (unsigned long long)ph[1],
                 (unsigned long long)ph[2], (unsigned long long)ph[3],
                 (unsigned long long)ph[4], (unsigned long long)ph[5]);
  }
  out->n_selected = h->pending_n_sel;
  out->iteration = res.iteration;
  out->has_peak = 1;
  out->peak = res.peak;
  out->diverging = res.diverging;
  out->flux_cleaned = res.flux;
  if (h_trace && trace_cap && trace_dev) {
    const uint64_t n = std::min<uint64_t>(res.iteration - h->pending_start, trace_cap);
    RDL_HIP_CHECK(hipMemcpyAsync(h_trace, trace_dev, n * 8,
                                 hipMemcpyDeviceToHost, st));
    RDL_HIP_CHECK(hipStreamSynchronize(st));
  }
  return RDL_OK;
}
}  // namespace

}  // extern "C"
