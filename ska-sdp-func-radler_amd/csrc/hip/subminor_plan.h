// Which sub-minor loop kernel runs, and how the selection is laid out for it:
// a pure host function of the tuning and a dozen integers, so the choice can
// be read in one piece and tested without a GPU (tests/test_subminor_plan.py
// compares it with recorded results over its whole domain). Plain C++17;
// nothing from HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "rdl_hip.h"

namespace rdl {

// rdl_subminor_set_tuning and the RDL_SUBMINOR_* switches
struct SubminorTuning {
  int mode = 0;  // 0 auto, 1 LDS kernel, 2 register kernel, 3 single-wave kernel,
                 // 4 one 1024-thread workgroup, 5 1024-thread grid, 6 table kernel
  uint32_t target_per_block = 1024;  // pixels per workgroup (multi-workgroup)
  uint32_t single_max = 2048;        // largest selection kept on one workgroup
  uint32_t wave_max = 128;           // largest selection on the single-wave kernel
  uint32_t big_max = 3584;           // largest selection on one 1024-thread workgroup
  uint32_t big_target = 0;           // > 0: larger selections on 1024-thread grids
  uint32_t table_max = 16384;        // largest selection given a pairwise PSF table
  int tab = 1;                       // SubminorLoopTab where it applies (RDL_SUBMINOR_TAB=0: off)
  uint32_t tab_target = 1024;        // pixels per participant (RDL_SUBMINOR_TAB_TARGET)
  uint32_t tab_single = 8192;        // one workgroup up to this (RDL_SUBMINOR_TAB_SINGLE)
  uint32_t tab_threads = 0;          // 0: 256 up to 2048 pixels per participant, else 512
};

// what the choice depends on, of one launch
struct SubminorShape {
  uint64_t n_sel = 0;  // selected pixels (>= 1)
  uint32_t n_images = 1, n_pol = 1;
  uint32_t integ_mode = RDL_INTEGRATE_LINEAR;
  bool copy_fast_path = false;  // one image whose integration is the identity
  bool has_rms = false, has_spectral = false, has_logpoly = false;
  int n_cus = 256;
  uint32_t coop_limit = 0;  // cap on cooperative grids (0: n_cus)
};

enum class LoopKind {
  Lds,   // SubminorLoop<NI>
  Reg,   // SubminorLoopReg<NI, ITEMS, FAST, 512>
  Wave,  // SubminorLoopReg<NI, ITEMS, FAST, 64>
  Big,   // SubminorLoopReg<NI, ITEMS, FAST, 1024>
  Tab,   // SubminorLoopTab<ITEMS, THREADS, NEG>
  TabN   // SubminorLoopTabN<NI, ITEMS, 256, NEG>
};

struct LoopPlan {
  LoopKind kind = LoopKind::Lds;
  uint32_t threads = 0;      // workgroup size
  uint32_t items = 0;        // pixels per thread (the kernel's ITEMS; 0: Lds)
  uint32_t n_blocks = 0;     // workgroups (table kernels: participants)
  uint64_t per_block = 0;    // pixels per workgroup
  bool use_lds = false;      // Lds: the selection fits the workgroups' LDS
  size_t lds_bytes = 0;      //   and its dynamic LDS per workgroup
  bool build_table = false;  // the loop reads the pairwise PSF table
  uint32_t part_stride = 0;  // LoopArgs::part_stride
  size_t rec_bytes = 0;      // the exchange records of all workgroups
  uint32_t ni_template = 0;  // NI of the register and LDS kernels
  int trace_kind = 0;        // kind= of the RDL_TRACE_SUBMINOR line
  int error = RDL_OK;        // RDL_OK or RDL_ERR_ARG
  const char* error_text = nullptr;
};

constexpr uint32_t kLoopThreads = 512;
constexpr uint32_t kRegThreads = 512;
constexpr uint32_t kTabParticipantStride = 8;  // blocks per participant (LoopArgs::part_stride)

// Register budget: ITEMS x N_img residuals + model values + gathers per lane.
constexpr uint32_t RegMaxItems(uint32_t ni) {
  return ni <= 2 ? 8 : ni <= 4 ? 4 : 2;
}

// Single-wave register budget: ITEMS x N_img residuals + model values +
// gathers per lane.
constexpr uint32_t WaveMaxItems(uint32_t ni) {
  return ni <= 1 ? 16 : ni <= 2 ? 8 : ni <= 4 ? 4 : 2;
}

namespace plan {

constexpr uint64_t CeilDiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// the instantiated ITEMS (powers of two up to `most`) that hold `need`
constexpr uint32_t ItemsFor(uint64_t need, uint32_t most) {
  uint32_t items = 1;
  while (items < most && items < need) items *= 2;
  return items;
}

// n_sel pixels over g workgroups
struct Partition {
  uint32_t g;
  uint64_t per;
};
constexpr Partition Split(uint64_t n_sel, uint32_t g) { return {g, CeilDiv(n_sel, g)}; }

inline LoopPlan Fail(const char* text) {
  LoopPlan p;
  p.error = RDL_ERR_ARG;
  p.error_text = text;
  return p;
}

}  // namespace plan

inline LoopPlan PlanSubminorLoop(const SubminorTuning& t, const SubminorShape& s) {
  using plan::CeilDiv;
  using plan::ItemsFor;
  using plan::Partition;
  using plan::Split;
  const uint64_t n_sel = s.n_sel;
  const uint32_t ni = s.n_images;
  const int mode = t.mode;
  const uint32_t n_cus = uint32_t(std::max(1, std::min(s.n_cus, 256)));
  const uint32_t max_blocks = s.coop_limit ? std::min(n_cus, s.coop_limit) : n_cus;
  // register kernel: N_img <= 8, <= 4096 pixels per workgroup
  const uint32_t ni_t = ni <= 1 ? 1 : ni <= 2 ? 2 : ni <= 4 ? 4 : 8;
  // the log-polynomial fit runs in the LDS-resident loop only
  const bool lpfit = s.has_logpoly;
  const bool reg_ok = ni <= 8 && !lpfit;
  const uint64_t reg_cap = uint64_t(kRegThreads) * RegMaxItems(ni_t);
  // the size limits count PSF gathers per iteration (pixels x images): with
  // joined channels one workgroup's memory pipe, not the exchange, bounds an
  // iteration (8 channels x 3000 pixels on one CU: 26 us per component)
  const uint64_t work = n_sel * ni;
  // with the pairwise table an iteration reads one contiguous row per PSF:
  // one workgroup (up to 1024 threads) then holds selections that would
  // otherwise pay a cross-workgroup exchange per component
  const uint64_t big_cap = 1024ull * (ni_t <= 2 ? 8 : 4);
  const bool want_table = (mode == 0 || mode == 6) && reg_ok && n_sel >= 2 &&
                          n_sel <= t.table_max &&
                          uint64_t(ni / s.n_pol) * n_sel * n_sel <=
                              (uint64_t(1) << (ni > 1 ? 29 : 28));  // 1 / 2 GiB
  // (one CU's memory pipe streams those rows: at most 8192 values per
  // iteration, so joined channels keep the grid above 8192 / N_img pixels)
  const bool table_single = want_table && n_sel <= big_cap && work <= 8192;

  // ---- 512-thread register kernel: one workgroup, or a grid of about
  // target_per_block pixels x images each (at least two workgroups)
  const bool reg_wanted = reg_ok && mode != 1;
  const bool reg_splits =
      reg_wanted && !table_single && (n_sel > reg_cap || work > t.single_max);
  const uint64_t reg_target =
      std::max<uint64_t>(std::max<uint32_t>(t.target_per_block, 512) / ni, 64);
  const Partition reg_part =
      reg_splits ? Split(n_sel, std::max<uint32_t>(
                                    uint32_t(std::min<uint64_t>(max_blocks,
                                                                CeilDiv(n_sel, reg_target))),
                                    std::min<uint32_t>(2, max_blocks)))
                 : Partition{1, n_sel};
  const bool reg_holds = reg_wanted && (!reg_splits || reg_part.per <= reg_cap);
  if (!reg_holds && (mode == 2 || mode == 3))
    return plan::Fail("register sub-minor kernel cannot hold this selection");

  // ---- single wave: no barrier and no LDS exchange per iteration
  const uint64_t wave_cap = 64ull * WaveMaxItems(ni_t);
  const bool use_wave = reg_holds && reg_part.g == 1 &&
                        ((mode == 0 && n_sel <= wave_cap && work <= t.wave_max) ||
                         (mode == 3 && n_sel <= wave_cap));
  if (mode == 3 && !use_wave)
    return plan::Fail("single-wave sub-minor kernel cannot hold this selection");

  // ---- one sixteen-wave workgroup (mode 4 forces it)
  const bool big_single =
      !use_wave && reg_ok && mode != 1 && mode != 2 &&
      ((mode == 0 && n_sel <= big_cap &&
        ((work <= t.big_max && work > 1024) || (table_single && n_sel > 1024))) ||
       (mode == 4 && n_sel <= big_cap));
  // ---- 1024-thread workgroups on a cooperative grid (mode 5, target pixels
  // per workgroup from set_tuning; mode 0 when big_target is set)
  const bool big_grid_wanted =
      !use_wave && !big_single && reg_ok &&
      (mode == 5 || (mode == 0 && t.big_target > 0 && n_sel > t.big_max));
  const uint64_t big_target =
      mode == 5 ? std::max<uint32_t>(t.target_per_block, 1024) : std::max<uint32_t>(t.big_target, 1);
  const Partition big_part = Split(
      n_sel,
      std::max<uint32_t>(uint32_t(std::min<uint64_t>(max_blocks, CeilDiv(n_sel, big_target))), 1));
  const bool big_grid = big_grid_wanted && big_part.per <= big_cap;
  if (mode == 4 && !big_single)
    return plan::Fail("1024-thread sub-minor kernel cannot hold this selection");
  const bool use_big = big_single || big_grid;
  const bool use_reg = use_big || reg_holds;

  // ---- LDS kernel, when the registers cannot hold the selection: workgroups
  // of 4096 pixels, else every workgroup there is; global scratch when even
  // those outgrow 150 KiB of LDS each
  const size_t bytes_per_px = 4 + 8 * size_t(ni);
  const size_t lds_cap = 150 * 1024;
  const Partition lds_first =
      Split(n_sel, n_sel <= 4096 ? 1u : uint32_t(std::min<uint64_t>(max_blocks, CeilDiv(n_sel, 4096))));
  const Partition lds_part =
      lds_first.per * bytes_per_px <= lds_cap ? lds_first : Split(n_sel, max_blocks);
  // (a table kernel chosen below ignores use_lds)
  const bool use_lds = !use_reg && lds_part.per * bytes_per_px <= lds_cap;

  // ---- the partition without a table kernel, and the 512-thread ITEMS
  const Partition base = big_single ? Partition{1, n_sel}
                         : big_grid ? big_part
                         : use_reg  ? reg_part
                                    : lds_part;
  const uint32_t reg_items = use_reg ? ItemsFor(CeilDiv(base.per, kRegThreads), 8) : 0;

  // ---- the pairwise-table loop (mode 6 forces it): one image, identity
  // integration, no RMS / spectral / log-polynomial fit; participants of
  // about tab_target pixels each (one workgroup up to tab_target)
  const bool tab_shape = want_table && ni == 1 && s.copy_fast_path && !s.has_rms &&
                         !s.has_spectral && !lpfit;
  const bool use_tab =
      tab_shape && ((mode == 0 && t.tab) || mode == 6) && !(mode == 0 && use_wave);
  if (mode == 6 && !use_tab)
    return plan::Fail("table sub-minor kernel does not apply to this selection");

  LoopPlan p;
  p.ni_template = ni_t;
  p.use_lds = use_lds;
  p.lds_bytes = use_lds ? lds_part.per * bytes_per_px : 0;

  // ---- joined images (2..8, no RMS / spectral / log-polynomial fit):
  // SubminorLoopTabN, participants of up to 1024 pixels (a row of every PSF
  // per pixel: 1024 x 8 PSFs is the 32 KiB an iteration of one workgroup
  // streams), at most 32 (one XCD)
  const bool tabn_shape = want_table && ni > 1 && ni <= 8 && !s.has_rms && !s.has_spectral &&
                          !lpfit && t.tab && mode == 0 && !use_wave &&
                          s.integ_mode == RDL_INTEGRATE_LINEAR && !s.copy_fast_path &&
                          s.n_pol == 1;
  const uint64_t tabn_target = std::min<uint64_t>(
      std::max<uint64_t>(256, 8192 / std::max<uint32_t>(ni / s.n_pol, 1)), 1024);
  const uint64_t tabn_g = CeilDiv(n_sel, tabn_target);
  const bool use_tabn = tabn_shape && tabn_g <= std::min<uint32_t>(32, max_blocks);

  if (use_tab) {
    // one workgroup up to 8192 pixels (measured on MI355X: an exchange costs
    // more than the row it splits below that; tools/bench_subminor.py), then
    // participants of tab_target pixels; mode 6 always splits by tab_target
    const uint64_t target = mode == 6 || n_sel > t.tab_single
                                ? std::max<uint32_t>(t.tab_target, 256)
                                : std::max<uint64_t>(n_sel, 1);
    const Partition part = Split(
        n_sel, std::max<uint32_t>(
                   uint32_t(std::min<uint64_t>({CeilDiv(n_sel, target), 32, max_blocks})), 1));
    // measured on MI355X (tools/bench_subminor.py, RDL_BENCH_TAB): four
    // waves up to 2048 pixels and for grid participants, eight to 8192
    const uint32_t asked = t.tab_threads == 256 || t.tab_threads == 512 || t.tab_threads == 1024
                               ? t.tab_threads
                               : (part.g > 1 || part.per <= 2048 ? 256u : 512u);
    // (ITEMS goes to 32 with 256 threads, to 16 with more)
    const uint32_t threads =
        CeilDiv(part.per, asked) > (asked == 256 ? 32u : 16u) ? 1024u : asked;
    const uint64_t need = CeilDiv(part.per, threads);
    if (need > (threads == 256 ? 32u : 16u))
      return plan::Fail("table sub-minor kernel: too many pixels per participant");
    p.kind = LoopKind::Tab;
    p.threads = threads;
    p.items = ItemsFor(need, 32);
    p.n_blocks = part.g;
    p.per_block = part.per;
    p.trace_kind = 30 + int(p.items);
    p.rec_bytes = (size_t(7) * part.g * sizeof(uint64_t) + 15) / 16 * 16;
  } else if (use_tabn) {
    const Partition part = Split(n_sel, uint32_t(std::max<uint64_t>(tabn_g, 1)));
    p.kind = LoopKind::TabN;
    p.threads = 256;
    p.items = ItemsFor(CeilDiv(part.per, 256), 4);
    p.n_blocks = part.g;
    p.per_block = part.per;
    p.trace_kind = 50 + int(p.items);
    p.rec_bytes = ((size_t(1) + 2 * (3 + ni)) * part.g * sizeof(uint64_t) + 15) / 16 * 16;
  } else if (use_reg) {
    p.kind = use_big ? LoopKind::Big : use_wave ? LoopKind::Wave : LoopKind::Reg;
    p.threads = use_big ? 1024 : use_wave ? 64 : kRegThreads;
    p.items = use_big    ? ItemsFor(CeilDiv(base.per, 1024), 8)
              : use_wave ? ItemsFor(CeilDiv(n_sel, 64), 16)
                         : reg_items;
    p.n_blocks = base.g;
    p.per_block = base.per;
    p.trace_kind = 10 + int(reg_items);
    p.rec_bytes = (size_t(2) * base.g * (3 + ni_t) * sizeof(uint64_t) + 15) / 16 * 16;
  } else {
    const uint32_t rec_words = (4 + ni + 3) / 4 * 4;  // LoopArgs::rec_words
    p.kind = LoopKind::Lds;
    p.threads = kLoopThreads;
    p.n_blocks = base.g;
    p.per_block = base.per;
    p.trace_kind = int(use_lds);
    p.rec_bytes = size_t(2) * base.g * rec_words * sizeof(uint32_t);
  }
  // the table and the epoch-tagged granules belong to every kernel but Lds
  p.build_table = p.kind != LoopKind::Lds && want_table;
  // a pooled session (coop_limit: its share of the CUs) launches only as
  // many blocks as its share; the participants then spread over XCDs and
  // exchange through agent-scope stores (the kernel sees the XCC ids)
  const bool spread = (use_tab || use_tabn) && p.n_blocks > 1 && s.coop_limit &&
                      uint64_t(p.n_blocks) * kTabParticipantStride > s.coop_limit;
  p.part_stride = spread ? 1 : kTabParticipantStride;
  return p;
}

}  // namespace rdl
