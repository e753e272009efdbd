// Line references are to the reference's
// cpp/algorithms/parallel_deconvolution.cc.
#include "parallel_deconvolution.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cmath>
#include <cstdlib>
#include <exception>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>

#include "host_profile.h"
#include "logger.h"
#include "multiscale_algorithm.h"

namespace radler::algorithms {

ParallelDeconvolution::ParallelDeconvolution(const Settings& settings)
    : settings_(settings) {}

ParallelDeconvolution::~ParallelDeconvolution() = default;

const DeconvolutionAlgorithm& ParallelDeconvolution::MaxScaleCountAlgorithm()
    const {
  if (settings_.algorithm_type == AlgorithmType::kMultiscale) {
    const auto* best =
        static_cast<const MultiScaleAlgorithm*>(algorithms_.front().get());
    for (size_t i = 1; i != algorithms_.size(); ++i) {
      const auto* a = static_cast<const MultiScaleAlgorithm*>(algorithms_[i].get());
      if (a->ScaleCount() > best->ScaleCount()) best = a;
    }
    return *best;
  }
  return FirstAlgorithm();
}

void ParallelDeconvolution::SetAlgorithm(
    std::unique_ptr<DeconvolutionAlgorithm> algorithm) {  // :227-242
  algorithms_.resize(settings_.parallel.grid_width *
                     settings_.parallel.grid_height);
  algorithms_.front() = std::move(algorithm);
  for (size_t i = 1; i != algorithms_.size(); ++i)
    algorithms_[i] = algorithms_.front()->Clone();
}

void ParallelDeconvolution::SetThreshold(double threshold) {
  for (auto& a : algorithms_) a->SetThreshold(threshold);
}

void ParallelDeconvolution::SetMinorLoopGain(double gain) {
  for (auto& a : algorithms_) a->SetMinorLoopGain(gain);
}

void ParallelDeconvolution::SetAutoMaskMode(bool track_per_scale_masks,
                                            bool use_per_scale_masks) {
  track_masks_ = track_per_scale_masks;
  use_masks_ = use_per_scale_masks;
  for (auto& a : algorithms_)
    if (auto* ms = dynamic_cast<MultiScaleAlgorithm*>(a.get()))
      ms->SetAutoMaskMode(track_per_scale_masks, use_per_scale_masks);
}

void ParallelDeconvolution::LoadScaleMasks(const SubImage& sub, size_t width) {
  if (!use_masks_ && !track_masks_) return;
  auto* ms = dynamic_cast<MultiScaleAlgorithm*>(algorithms_[sub.index].get());
  if (!ms) return;
  const std::lock_guard<std::mutex> lock(masks_mutex_);
  if (scale_masks_.empty()) return;
  ms->SetScaleMaskCount(std::max(ms->GetScaleMaskCount(), scale_masks_.size()));
  for (size_t i = 0; i != ms->GetScaleMaskCount(); ++i) {
    std::vector<uint8_t>& m = ms->GetScaleMask(i);
    m.assign(sub.width * sub.height, 0);
    if (i >= scale_masks_.size()) continue;
    // scale mask box AND the subimage's clean mask (:376-386)
    for (size_t y = 0; y != sub.height; ++y)
      for (size_t x = 0; x != sub.width; ++x) {
        const size_t p = y * sub.width + x;
        m[p] = (scale_masks_[i][(sub.y + y) * width + sub.x + x] && sub.mask[p]) ? 1 : 0;
      }
  }
}

std::vector<std::vector<uint8_t>> ParallelDeconvolution::SubImageScaleMasks(
    const SubImage& sub) {
  std::vector<std::vector<uint8_t>> out;
  auto* ms = dynamic_cast<MultiScaleAlgorithm*>(algorithms_[sub.index].get());
  if (!ms) return out;
  for (size_t i = 0; i != ms->ScaleCount() && i != ms->GetScaleMaskCount(); ++i)
    out.push_back(ms->GetScaleMask(i));
  return out;
}

void ParallelDeconvolution::StoreScaleMasks(
    const SubImage& sub, size_t width, size_t height,
    const std::vector<std::vector<uint8_t>>& sub_masks) {
  const std::lock_guard<std::mutex> lock(masks_mutex_);
  if (scale_masks_.empty())
    scale_masks_.assign(sub_masks.size(), std::vector<uint8_t>(width * height, 0));
  for (size_t i = 0; i != sub_masks.size() && i != scale_masks_.size(); ++i)
    for (size_t y = 0; y != sub.height; ++y)
      for (size_t x = 0; x != sub.width; ++x) {
        const size_t p = y * sub.width + x;
        if (sub.boundary_mask[p])
          scale_masks_[i][(sub.y + y) * width + sub.x + x] = sub_masks[i][p];
      }
}

void ParallelDeconvolution::SetRmsFactorImage(
    std::shared_ptr<const std::vector<float>> image, size_t width) {
  if (algorithms_.size() == 1) {
    algorithms_.front()->SetRmsFactorImage(std::move(image));
  } else {
    rms_image_ = std::move(image);
    rms_width_ = width;
  }
}

void ParallelDeconvolution::SetSpectrallyForcedImages(
    std::vector<std::vector<float>> planes, size_t width) {
  // the first algorithm validates and packs the planes; the others share them
  algorithms_.front()->SetSpectrallyForcedImages(std::move(planes), width);
  if (algorithms_.size() != 1)
    forced_images_ = algorithms_.front()->SpectrallyForcedImages();
}

void ParallelDeconvolution::SetCleanMask(const bool* mask) {
  if (algorithms_.size() == 1)
    algorithms_.front()->SetCleanMask(mask);
  else
    mask_ = mask;
}

ParallelDeconvolutionResult ParallelDeconvolution::ExecuteMajorIteration(
    ImageSet& data_image, ImageSet& model_image,
    const std::vector<gpu::Planes>& psf_images,
    const std::vector<PsfOffset>& psf_offsets, double major_loop_gain) {
  if (algorithms_.size() == 1)
    return ExecuteSingleThreadedRun(data_image, model_image, psf_images,
                                    psf_offsets, major_loop_gain);
  return ExecuteParallelRun(data_image, model_image, psf_images, psf_offsets,
                            major_loop_gain);
}

ParallelDeconvolutionResult ParallelDeconvolution::ExecuteSingleThreadedRun(
    ImageSet& data_image, ImageSet& model_image,
    const std::vector<gpu::Planes>& psf_images,
    const std::vector<PsfOffset>& psf_offsets, double major_loop_gain) {
  // :510-553
  DeconvolutionAlgorithm& algorithm = *algorithms_.front();
  // one image set over the ranks: joined channels are shared by channel
  // (MultiScaleAlgorithm::SetChannelShard)
  algorithm.SetChannelShard(comm_ && comm_->Size() > 1 ? comm_.get() : nullptr);
  const size_t psf_index = NearestPsfIndex(
      psf_offsets, model_image.Width() / 2, model_image.Height() / 2);
  const gpu::Planes& psfs = psf_images[psf_index];
  algorithm.SetMajorLoopGain(major_loop_gain);
  DeconvolutionResult result;
  if (psfs.width == data_image.Width() && psfs.height == data_image.Height()) {
    result = algorithm.ExecuteMajorIteration(data_image, model_image, psfs);
  } else {
    // DD-PSFs smaller than the image: Image::Untrim to the image size
    if (psfs.width > data_image.Width() || psfs.height > data_image.Height())
      throw std::runtime_error("PSF larger than the image");
    gpu::Session& s = data_image.Session();
    gpu::Planes resized = gpu::Planes::Make(s, data_image.Width(),
                                            data_image.Height(), psfs.count);
    for (size_t i = 0; i != psfs.count; ++i)
      gpu::Check(rdl_untrim(s.Handle(), resized.Plane(i),
                            uint32_t(data_image.Width()),
                            uint32_t(data_image.Height()), psfs.Plane(i),
                            uint32_t(psfs.width), uint32_t(psfs.height)),
                 "rdl_untrim");
    result = algorithm.ExecuteMajorIteration(data_image, model_image, resized);
  }
  ParallelDeconvolutionResult global;
  global.another_iteration_required = result.another_iteration_required;
  global.start_peak = result.starting_peak_value;
  global.end_peak = result.final_peak_value;
  return global;
}

namespace {

// The boundary mask of `sub` as bytes on the device of `s`.
gpu::Buffer UploadBoundary(gpu::Session& s, const SubImage& sub) {
  const std::vector<uint8_t> bytes(sub.boundary_mask.begin(), sub.boundary_mask.end());
  gpu::Buffer d_mask(s, bytes.size());
  s.H2D(d_mask.Ptr(), bytes.data(), bytes.size());
  return d_mask;
}

// ImageSet::Trim / TrimMasked of the data and model planes and the centred
// Image::Resize of the PSFs into contiguous subimage planes, as box copies
// ordered on `ops` (parallel_deconvolution.cc:300-357)
void TrimSubImage(gpu::Session& ops, const SubImage& sub, const ImageSet& data_image,
                  const ImageSet& model_image, const gpu::Planes& psfs,
                  float* d_data, float* d_model, float* d_psfs,
                  const uint8_t* d_boundary) {
  prof::Section prof_section("par.trim");
  const size_t W = data_image.Width();
  const uint32_t uw = uint32_t(sub.width), uh = uint32_t(sub.height);
  const size_t n = sub.width * sub.height;
  for (size_t i = 0; i != data_image.Size(); ++i) {
    gpu::Check(rdl_box(ops.Handle(), d_data + i * n, uw, 0, 0, data_image.Data(i),
                       uint32_t(W), uint32_t(sub.x), uint32_t(sub.y), uw, uh,
                       nullptr, RDL_BOX_COPY),
               "rdl_box");  // ImageSet::Trim
    gpu::Check(rdl_box(ops.Handle(), d_model + i * n, uw, 0, 0, model_image.Data(i),
                       uint32_t(W), uint32_t(sub.x), uint32_t(sub.y), uw, uh,
                       d_boundary, RDL_BOX_COPY_ZERO),
               "rdl_box");  // ImageSet::TrimMasked
  }
  // Image::Resize (:323-330), centred per axis: a PSF larger than the
  // subimage is cropped, a smaller one (a fine DD-PSF grid) zero-padded
  const size_t cw = std::min(psfs.width, sub.width), ch = std::min(psfs.height, sub.height);
  const size_t src_x = (psfs.width - cw) / 2, src_y = (psfs.height - ch) / 2;
  const size_t dst_x = (sub.width - cw) / 2, dst_y = (sub.height - ch) / 2;
  if (cw != sub.width || ch != sub.height) ops.Zero(d_psfs, psfs.count * n * sizeof(float));
  for (size_t i = 0; i != psfs.count; ++i)
    gpu::Check(rdl_box(ops.Handle(), d_psfs + i * n, uw, uint32_t(dst_x), uint32_t(dst_y),
                       psfs.Plane(i), uint32_t(psfs.width), uint32_t(src_x),
                       uint32_t(src_y), uint32_t(cw), uint32_t(ch), nullptr, RDL_BOX_COPY),
               "rdl_box");
}

// ImageSet::CopyMasked of the residual (only when the subimage converged) and
// ImageSet::AddSubImage of the model (parallel_deconvolution.cc:458-484)
void MergeSubImage(gpu::Session& ops, const SubImage& sub, ImageSet& data_image,
                   ImageSet& result_model, const float* d_data,
                   const float* d_model, const uint8_t* d_boundary,
                   bool converging) {
  prof::Section prof_section("par.merge");
  const size_t W = data_image.Width();
  const uint32_t uw = uint32_t(sub.width), uh = uint32_t(sub.height);
  const size_t n = sub.width * sub.height;
  for (size_t i = 0; i != data_image.Size(); ++i) {
    if (converging)
      gpu::Check(rdl_box(ops.Handle(), data_image.Data(i), uint32_t(W),
                         uint32_t(sub.x), uint32_t(sub.y), d_data + i * n, uw, 0, 0,
                         uw, uh, d_boundary, RDL_BOX_COPY_MASKED),
                 "rdl_box");
    gpu::Check(rdl_box(ops.Handle(), result_model.Data(i), uint32_t(W),
                       uint32_t(sub.x), uint32_t(sub.y), d_model + i * n, uw, 0, 0,
                       uw, uh, nullptr, RDL_BOX_ADD),
               "rdl_box");
  }
}

}  // namespace

bool ParallelDeconvolution::DeconvolveSubImage(SubImage& sub, ImageSet& sub_data,
                                               ImageSet& sub_model,
                                               const gpu::Planes& sub_psfs,
                                               double major_iteration_threshold,
                                               bool find_peak_only) {
  // parallel_deconvolution.cc:363-456
  DeconvolutionAlgorithm& alg = *algorithms_[sub.index];
  std::vector<char> mask_copy(sub.mask.begin(), sub.mask.end());
  alg.SetCleanMask(reinterpret_cast<const bool*>(mask_copy.data()));
  if (rms_image_) {  // rms_image_.TrimBox (:332-337)
    auto sub_rms = std::make_shared<std::vector<float>>(sub.width * sub.height);
    for (size_t y = 0; y != sub.height; ++y)
      std::copy_n(rms_image_->data() + (sub.y + y) * rms_width_ + sub.x, sub.width,
                  sub_rms->data() + y * sub.width);
    alg.SetRmsFactorImage(std::move(sub_rms));
  }
  // the full-image term planes with this subimage's origin (:340-349)
  if (forced_images_) alg.SetSpectrallyForcedImages(forced_images_, sub.x, sub.y);
  const size_t max_n_iter = alg.MaxIterations();
  if (find_peak_only)
    alg.SetMaxIterations(0);
  else
    alg.SetMajorIterationThreshold(float(major_iteration_threshold));
  const double peak_at_start = std::fabs(sub.peak);
  const DeconvolutionResult result =
      alg.ExecuteMajorIteration(sub_data, sub_model, sub_psfs);
  alg.SetCleanMask(nullptr);
  if (rms_image_) alg.SetRmsFactorImage(nullptr);  // :421-423
  sub.peak = result.final_peak_value;
  sub.reached_major_threshold = result.another_iteration_required;
  const bool converging =
      (settings_.divergence_limit == 0.0 ||
       std::fabs(sub.peak) <= peak_at_start * settings_.divergence_limit) &&
      std::isfinite(sub.peak) && !result.is_diverging;
  if (find_peak_only) {
    alg.SetMaxIterations(max_n_iter);
  } else if (!converging) {
    log::Warn() << "Peak of sub-image " << sub.index << " increased from "
                << peak_at_start << " to " << sub.peak
                << " and deconvolution probably diverged: resetting.\n";
    sub.reached_major_threshold = false;
  }
  // :464-479: a converging multiscale subimage's components join the
  // full-image list at the subimage offset
  if (!find_peak_only && settings_.save_source_list && algorithms_.size() > 1 &&
      settings_.algorithm_type == AlgorithmType::kMultiscale) {
    auto& ms = static_cast<MultiScaleAlgorithm&>(alg);
    if (converging && ms.HasComponentList()) {
      const std::lock_guard<std::mutex> lock(masks_mutex_);
      if (!component_list_)
        component_list_ = std::make_unique<ComponentList>(
            settings_.trimmed_image_width, settings_.trimmed_image_height,
            ms.ScaleCount(), sub_data.Size());
      component_list_->Add(ms.GetComponentList(), int(sub.x), int(sub.y));
    }
    ms.ClearComponentList();
  }
  return converging;
}

ComponentList ParallelDeconvolution::GetMultiscaleComponentList() const {
  // :184-196: the single algorithm's list, or the merged subimage lists
  ComponentList list;
  if (algorithms_.size() == 1) {
    const auto& ms = static_cast<const MultiScaleAlgorithm&>(*algorithms_.front());
    if (ms.HasComponentList()) list = ms.GetComponentList();
  } else if (component_list_) {
    list = *component_list_;
  }
  list.MergeDuplicates();
  return list;
}

// One pass (find the start peaks, or clean) over the subimages.
struct ParallelDeconvolution::Pass {
  ImageSet& data_image;
  const ImageSet& model_image;
  ImageSet& result_model;
  const std::vector<gpu::Planes>& psf_images;
  const std::vector<size_t>& psf_indices;
  double threshold;             // the major iteration's (cleaning pass)
  bool find_peak_only, pooled;  // pooled: the subimages run on the worker pool
  gpu::Session& Main() const { return data_image.Session(); }
  const gpu::Planes& Psfs(const SubImage& s) const { return psf_images[psf_indices[s.index]]; }
};

// One subimage's device planes, box copies of the full image set's, through a pass.
struct ParallelDeconvolution::SubImageRun {
  SubImage* sub = nullptr;
  gpu::Buffer boundary;  // on the main device
  // main-device copy (data | model | psfs) of a staged run's planes, else unallocated
  gpu::Buffer stage;
  size_t set_floats = 0;  // of the data planes, and of the model planes
  std::unique_ptr<ImageSet> data, model, initial;
  gpu::Planes psfs;
  bool converging = false;

  const uint8_t* Boundary() const { return static_cast<const uint8_t*>(boundary.Ptr()); }
  float* Stage(size_t set) const { return stage.F() + set * set_floats; }
  const float* ModelToAdd() const { return (converging ? model : initial)->Base(); }

  // On the main session, before any worker starts; a staged run's planes are trimmed.
  void Begin(const Pass& pass, SubImage& subimage, bool staged) {
    sub = &subimage;
    const size_t n = sub->width * sub->height;
    set_floats = pass.data_image.Size() * n;
    boundary = UploadBoundary(pass.Main(), *sub);
    if (!staged) return;
    const size_t floats = 2 * set_floats + pass.Psfs(*sub).count * n;
    stage = gpu::Buffer(pass.Main(), floats * sizeof(float));
    TrimSubImage(pass.Main(), *sub, pass.data_image, pass.model_image, pass.Psfs(*sub),
                 Stage(0), Stage(1), Stage(2), Boundary());
  }

  // The planes on the session that runs the subimage: trimmed there, or peer-copied.
  void Prepare(const Pass& pass, gpu::Session& ws) {
    const size_t sw = sub->width, sh = sub->height;
    const size_t set_bytes = set_floats * sizeof(float);
    const gpu::Planes& src_psfs = pass.Psfs(*sub);
    const int main_device = pass.Main().Device();
    data = std::make_unique<ImageSet>(pass.data_image, sw, sh, ws);
    model = std::make_unique<ImageSet>(pass.model_image, sw, sh, ws);
    psfs = gpu::Planes::Make(ws, sw, sh, src_psfs.count);
    if (stage.Ptr()) {
      ws.Peer(data->Base(), ws.Device(), Stage(0), main_device, set_bytes);
      ws.Peer(model->Base(), ws.Device(), Stage(1), main_device, set_bytes);
      ws.Peer(psfs.Base(), ws.Device(), Stage(2), main_device,
              src_psfs.count * sw * sh * sizeof(float));
    } else {
      TrimSubImage(ws, *sub, pass.data_image, pass.model_image, src_psfs, data->Base(),
                   model->Base(), psfs.Base(), Boundary());
    }
    if (!pass.find_peak_only) {  // what a diverging run falls back to
      initial = std::make_unique<ImageSet>(*model, sw, sh);
      initial->CopyFrom(*model);
    }
  }

  // Deconvolves on `ws`; a staged cleaning run's result goes back into the stage.
  void Run(ParallelDeconvolution& parent, const Pass& pass, gpu::Session& ws) {
    const size_t width = pass.data_image.Width(), set_bytes = set_floats * sizeof(float);
    parent.LoadScaleMasks(*sub, width);
    converging = parent.DeconvolveSubImage(*sub, *data, *model, psfs, pass.threshold,
                                           pass.find_peak_only);
    if (pass.find_peak_only) return;
    // boundary masks are disjoint: merging in any order gives one result
    if (parent.track_masks_ && converging)
      parent.StoreScaleMasks(*sub, width, pass.data_image.Height(),
                             parent.SubImageScaleMasks(*sub));
    if (!stage.Ptr()) return;
    const int main_device = pass.Main().Device();
    ws.Peer(Stage(0), main_device, data->Base(), ws.Device(), set_bytes);
    ws.Peer(Stage(1), main_device, ModelToAdd(), ws.Device(), set_bytes);
  }

  // The residual and the model to add, on the main device: to the sink, or merged.
  void Deliver(const Pass& pass, const SubImageSink& sink) const {
    const float* d_data = stage.Ptr() ? Stage(0) : data->Base();
    const float* d_model = stage.Ptr() ? Stage(1) : ModelToAdd();
    if (sink)
      sink(sub->index, d_data, d_model, converging);
    else
      MergeSubImage(pass.Main(), *sub, pass.data_image, pass.result_model, d_data,
                    d_model, Boundary(), converging);
  }
};

void ParallelDeconvolution::RunSubImagesInTurn(const Pass& pass,
                                               const std::vector<char>* run,
                                               const SubImageSink& sink) {
  gpu::Session& s = pass.Main();
  for (SubImage& sub : subimages_) {
    if (run && !(*run)[sub.index]) continue;
    prof::Section prof_section(pass.find_peak_only ? "par.run_subimage_findpeak"
                                                   : "par.run_subimage_clean");
    SubImageRun r;
    r.Begin(pass, sub, false);
    r.Prepare(pass, s);
    r.Run(*this, pass, s);
    if (pass.find_peak_only) continue;
    r.Deliver(pass, sink);
    if (!sink) s.Sync();
  }
}

std::vector<int> ParallelDeconvolution::PoolDevices(int main_device) {
  // RADLER_DEVICES="0,1,2,3" spreads the subimage workers over those GPUs;
  // by default they share the device of the image set
  std::vector<int> devices;
  const char* env = std::getenv("RADLER_DEVICES");
  int count = 0;
  if (env) gpu::Check(rdl_device_count(&count), "rdl_device_count");
  std::istringstream list(env ? env : "");
  for (std::string item; std::getline(list, item, ',');) {
    if (item.empty()) continue;
    const int d = std::stoi(item);
    if (d < 0 || d >= count)
      throw std::runtime_error("RADLER_DEVICES names device " + item +
                               ", which does not exist");
    devices.push_back(d);
  }
  if (devices.empty()) devices.push_back(main_device);
  return devices;
}

void ParallelDeconvolution::EnsureWorkers(gpu::Session& main, size_t n) {
  if (workers_.size() == n && worker_main_device_ == main.Device()) return;
  if (!workers_.empty())
    throw std::runtime_error(
        "ParallelDeconvolution: the subimage worker pool cannot change between "
        "major iterations");
  const std::vector<int> devices = PoolDevices(main.Device());
  std::map<int, size_t> per_device;
  for (size_t w = 0; w != n; ++w) {
    const int d = devices[w % devices.size()];
    workers_.push_back(gpu::Session::Worker(d, per_device[d]));
    ++per_device[d];
  }
  for (auto& w : workers_) w->SetConcurrency(per_device[w->Device()]);
  worker_main_device_ = main.Device();
  main.Bind();
}

double SubImageCost(size_t area, double peak, double threshold, bool find_peak_only) {
  const double thr = std::max(threshold, 1e-30);
  const double above = find_peak_only ? 1.0 : std::max(std::fabs(peak), thr) / thr;
  return double(area) * (1.0 + std::log2(above));
}

// The subimages' assignment to the pool's workers (on the main device):
//   0: fixed round robin (subimage k on worker k mod W);
//   1: one queue, the costliest first (the longest-processing-time rule:
//      the cleaning pass's estimate from the start peaks, as the ranks'
//      LptOwners; the find-peak pass by area);
//   2: one queue in index order (first free worker takes the next).
// Default: 1 for image sets of several images (joined channels), 0 for
// one image; RADLER_POOL_QUEUE overrides. Measured with the stream pool
// (r06, bench_legs.py, one job): 8 x 4096^2 joined split 8 x 8 — 0: 4.61-
// 4.63 s, 1: 3.91-4.08 s, 2: 4.15-4.38 s; 8192^2 split 8 x 8 — 0: 4.03-
// 4.08 s, 1: 4.17-4.23 s, 2: 4.17-4.46 s. Workers on other GPUs always
// keep the fixed assignment (their planes are staged on the main device
// before the pass). The result does not depend on the assignment (the
// snapshot schedule; tests/test_tiling.py::test_concurrent_pool_queue).
//   3: the cost order dealt round robin (worker w: the w-th, (w + W)-th, ...
//      costliest), a fixed assignment (measured: joined split 4.29-4.32 s, the
//      8192^2 split 4.12-4.41 s; neither default improves)
PoolAssignment AssignPool(int queue_mode, const std::vector<char>& worker_local,
                          bool force_staging, const std::vector<double>& costs,
                          const std::vector<char>* run) {
  const size_t W = worker_local.size();
  const bool all_local =
      !force_staging && queue_mode >= 1 && queue_mode <= 3 &&
      std::find(worker_local.begin(), worker_local.end(), 0) == worker_local.end();
  PoolAssignment plan;
  for (size_t i = 0; i != costs.size(); ++i)
    if (!run || (*run)[i]) plan.order.push_back(i);
  plan.staged.assign(costs.size(), 0);
  if (!all_local) {  // the fixed assignment: the k-th of them on worker k mod W
    for (size_t k = 0; k != plan.order.size(); ++k)
      plan.staged[plan.order[k]] = force_staging || !worker_local[k % W];
    return plan;
  }
  plan.shared_counter = queue_mode != 3;
  if (queue_mode != 2)
    std::stable_sort(plan.order.begin(), plan.order.end(),
                     [&](size_t a, size_t b) { return costs[a] > costs[b]; });
  return plan;
}

// AssignPool's mode (RADLER_POOL_QUEUE), and whether RADLER_POOL_STAGING=1 routes
// same-device workers through another GPU's staging and peer copies (one-GPU tests).
static std::pair<int, bool> ReadPoolSwitches(size_t n_images) {
  const char* queue = std::getenv("RADLER_POOL_QUEUE");
  const char* staging = std::getenv("RADLER_POOL_STAGING");
  const int mode = queue ? std::atoi(queue) : (n_images > 1 ? 1 : 0);
  return {mode, staging && staging[0] == '1'};
}

void ParallelDeconvolution::RunSubImagesConcurrently(const Pass& pass,
                                                     const std::vector<char>* run,
                                                     const SubImageSink& sink) {
  // The reference runs RunSubImage on settings.parallel.max_threads threads
  // (parallel_deconvolution.cc:583-616), each trimming from the shared
  // residual and copying back under a mutex. Here every subimage trims from
  // the residual as it was when the pass started and the copy-backs are
  // applied afterwards in subimage order: the schedule the reference takes
  // when all its threads trim before the first one finishes, made
  // deterministic. Boundary masks are disjoint and the model additions
  // outside them add zeros, so the merged result does not depend on the
  // number of workers or devices.
  gpu::Session& s = pass.Main();
  const size_t n_sub = subimages_.size(), W = workers_.size();
  const auto [queue_mode, force_staging] = ReadPoolSwitches(pass.data_image.Size());
  std::vector<char> worker_local(W);
  for (size_t w = 0; w != W; ++w) worker_local[w] = workers_[w]->Device() == s.Device();
  const double threshold = algorithms_.front()->Threshold();
  std::vector<double> costs;
  for (const SubImage& sub : subimages_)
    costs.push_back(
        SubImageCost(sub.width * sub.height, sub.peak, threshold, pass.find_peak_only));
  const PoolAssignment plan =
      AssignPool(queue_mode, worker_local, force_staging, costs, run);
  std::vector<size_t> todo = plan.order;  // in index order
  std::sort(todo.begin(), todo.end());
  std::vector<SubImageRun> runs(n_sub);
  for (const size_t i : todo) runs[i].Begin(pass, subimages_[i], plan.staged[i]);
  s.Sync();

  std::vector<std::exception_ptr> errors(W);
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};
  auto work = [&](size_t w) {
    try {
      gpu::Session& ws = *workers_[w];
      ws.Bind();
      const bool shared = plan.shared_counter;
      for (size_t k = shared ? next.fetch_add(1) : w; k < todo.size() && !failed;
           k = shared ? next.fetch_add(1) : k + W) {
        SubImageRun& r = runs[plan.order[k]];
        r.Prepare(pass, ws);
        r.Run(*this, pass, ws);
        ws.Sync();
        // only an unstaged cleaning run keeps its planes, for the merge
        if (pass.find_peak_only || r.stage.Ptr()) {
          r.data.reset(), r.model.reset(), r.initial.reset();
          r.psfs = gpu::Planes();
        }
      }
      ws.Sync();
    } catch (...) {
      errors[w] = std::current_exception();
      failed = true;
    }
  };
  std::vector<std::thread> threads;
  for (size_t w = 0; w != W; ++w) threads.emplace_back(work, w);
  for (std::thread& t : threads) t.join();
  s.Bind();
  for (std::exception_ptr& e : errors)
    if (e) std::rethrow_exception(e);
  if (pass.find_peak_only) return;
  for (const size_t i : todo) runs[i].Deliver(pass, sink);
  s.Sync();
}

double ParallelDeconvolution::RunSubImagesDistributed(const Pass& pass) {
  // The reference's threads (parallel_deconvolution.cc:583-616) become ranks:
  // subimage i runs on rank SubImageOwner(i). Every owned subimage trims from
  // the residual as it was when the pass started (the snapshot schedule of
  // RunSubImagesConcurrently), so the merged result is the same for any
  // number of ranks, and equal to the one-process pool's.
  gpu::Session& s = pass.Main();
  Communicator& comm = *comm_;
  const int rank = comm.Rank(), n_ranks = comm.Size();
  const size_t n_sub = subimages_.size(), n_img = pass.data_image.Size();
  // per subimage: a 64-byte record, then the residual and model planes
  struct Record {
    double peak;
    uint64_t iteration_number;
    uint32_t reached_major_threshold, converging;
    uint32_t n_mask_scales;  // tracked auto-masks that follow (second broadcast)
    uint32_t pad[9];
  };
  static_assert(sizeof(Record) == 64, "record layout");
  constexpr size_t kHeaderFloats = sizeof(Record) / sizeof(float);
  std::vector<std::unique_ptr<gpu::Buffer>> packs(n_sub);
  std::vector<std::vector<std::vector<uint8_t>>> mask_sets(n_sub);
  const bool lpt = !pass.find_peak_only && clean_owners_.size() == n_sub;
  auto owner_of = [&](size_t i) {
    return lpt ? clean_owners_[i] : SubImageOwner(i, n_ranks);
  };
  // a packed result: the record, then the residual and model boxes
  auto pack_result = [&](size_t i, const float* d_data, const float* d_model,
                         bool converging) {
    SubImage& sub = subimages_[i];
    const size_t n = sub.width * sub.height;
    auto pack = std::make_unique<gpu::Buffer>(
        s, (kHeaderFloats + 2 * n_img * n) * sizeof(float));
    Record rec{};
    rec.peak = sub.peak;
    rec.iteration_number = algorithms_[i]->IterationNumber();
    rec.reached_major_threshold = sub.reached_major_threshold ? 1u : 0u;
    rec.converging = converging ? 1u : 0u;
    if (track_masks_ && converging) {
      mask_sets[i] = SubImageScaleMasks(sub);
      rec.n_mask_scales = uint32_t(mask_sets[i].size());
    }
    s.H2D(pack->Ptr(), &rec, sizeof(rec));
    float* base = pack->F() + kHeaderFloats;
    s.D2D(base, d_data, n_img * n * sizeof(float));
    s.D2D(base + n_img * n, d_model, n_img * n * sizeof(float));
    packs[i] = std::move(pack);
  };
  // this rank's subimages: on its worker pool, or one after another
  std::vector<char> mine(n_sub, 0);
  for (size_t i = 0; i != n_sub; ++i) mine[i] = owner_of(i) == rank ? 1 : 0;
  if (pass.pooled)
    RunSubImagesConcurrently(pass, &mine, pack_result);
  else
    RunSubImagesInTurn(pass, &mine, pack_result);
  s.Sync();
  if (pass.find_peak_only) {
    // every rank gets every subimage's start peak (one RCCL allreduce(max)
    // of n_sub floats, the owners' entries against lowest()): the global
    // start peak (:592-599, signed, from 0.0) and the cost estimates of the
    // cleaning pass's ownership
    std::vector<float> peaks(n_sub, std::numeric_limits<float>::lowest());
    for (size_t i = 0; i != n_sub; ++i)
      if (SubImageOwner(i, n_ranks) == rank) peaks[i] = float(subimages_[i].peak);
    comm.AllreduceMax(s, peaks.data(), n_sub);
    double start_peak = 0.0;
    std::vector<double> costs(n_sub);
    for (size_t i = 0; i != n_sub; ++i) {
      SubImage& sub = subimages_[i];
      sub.peak = peaks[i];
      if (sub.peak > start_peak) start_peak = sub.peak;
      costs[i] = SubImageCost(sub.width * sub.height, sub.peak,
                              algorithms_.front()->Threshold(), false);
    }
    clean_owners_ = LptOwners(costs, n_ranks);
    return start_peak;
  }

  // copy-back (:458-484) in subimage order, identical on every rank
  std::unique_ptr<gpu::Buffer> staging;
  for (size_t i = 0; i != n_sub; ++i) {
    SubImage& sub = subimages_[i];
    const size_t n = sub.width * sub.height;
    const size_t bytes = (kHeaderFloats + 2 * n_img * n) * sizeof(float);
    const int owner = owner_of(i);
    gpu::Buffer* pack = packs[i].get();
    if (owner != rank) {
      if (!staging || staging->Bytes() < bytes)
        staging = std::make_unique<gpu::Buffer>(s, bytes);
      pack = staging.get();
    }
    comm.Broadcast(s, pack->Ptr(), bytes, owner);
    Record rec{};
    s.D2H(&rec, pack->Ptr(), sizeof(rec));
    if (owner != rank) {
      sub.peak = rec.peak;
      sub.reached_major_threshold = rec.reached_major_threshold != 0;
      algorithms_[i]->SetIterationNumber(size_t(rec.iteration_number));
    }
    const gpu::Buffer boundary = UploadBoundary(s, sub);
    const float* base = pack->F() + kHeaderFloats;
    MergeSubImage(s, sub, pass.data_image, pass.result_model, base, base + n_img * n,
                  static_cast<const uint8_t*>(boundary.Ptr()), rec.converging != 0);
    s.Sync();  // the staging buffer is reused by the next broadcast
    if (rec.n_mask_scales > 0) {  // the owner's tracked scale masks
      const size_t mb = size_t(rec.n_mask_scales) * n;
      gpu::Buffer dm(s, mb);
      if (owner == rank)
        for (size_t m = 0; m != rec.n_mask_scales; ++m)
          s.H2D(static_cast<uint8_t*>(dm.Ptr()) + m * n, mask_sets[i][m].data(), n);
      comm.Broadcast(s, dm.Ptr(), mb, owner);
      std::vector<std::vector<uint8_t>> masks(rec.n_mask_scales, std::vector<uint8_t>(n));
      for (size_t m = 0; m != rec.n_mask_scales; ++m)
        s.D2H(masks[m].data(), static_cast<const uint8_t*>(dm.Ptr()) + m * n, n);
      StoreScaleMasks(sub, pass.data_image.Width(), pass.data_image.Height(), masks);
    }
  }
  return 0.0;
}

double ParallelDeconvolution::RunPass(const Pass& pass) {
  // (the passes' wall clock: the part of a major iteration that the ranks
  // split; bench.py's Amdahl estimate)
  prof::Section prof_section(pass.find_peak_only ? "par.findpeak_pass"
                                                 : "par.clean_pass");
  // One worker: in index order, each seeing the copy-backs before it (the reference
  // with one thread). More (parallel.max_threads): concurrently on streams / GPUs.
  if (comm_) return RunSubImagesDistributed(pass);
  if (pass.pooled)
    RunSubImagesConcurrently(pass);
  else
    RunSubImagesInTurn(pass);
  double start_peak = 0.0;
  for (const SubImage& sub : subimages_)
    if (sub.peak > start_peak) start_peak = sub.peak;
  return start_peak;
}

ParallelDeconvolutionResult ParallelDeconvolution::ExecuteParallelRun(
    ImageSet& data_image, ImageSet& model_image,
    const std::vector<gpu::Planes>& psf_images,
    const std::vector<PsfOffset>& psf_offsets, double major_loop_gain) {
  // parallel_deconvolution.cc:556-654
  gpu::Session& s = data_image.Session();
  const size_t width = data_image.Width(), height = data_image.Height();
  std::vector<float> image(width * height);
  {
    gpu::Buffer integrated(s, width * height * sizeof(float));
    data_image.GetLinearIntegrated(integrated.F());
    s.D2H(image.data(), integrated.Ptr(), image.size() * sizeof(float));
  }
  std::vector<size_t> psf_indices;
  {
    prof::Section prof_split("par.split");
    subimages_ = MakeSubImages(image, width, height, mask_, psf_offsets, settings_,
                               psf_indices);
  }
  ImageSet result_model(model_image, width, height);
  result_model.Fill(0.0f);
  // settings.parallel.max_threads subimages in flight (:583-616), at most
  // kMaxStreams streams per GPU: beyond that the streams only share the
  // hardware queues (Settings' default is the host's processor count)
  constexpr size_t kMaxStreams = 16;
  const size_t n_workers =
      std::min<size_t>(std::min<size_t>(std::max<size_t>(settings_.parallel.max_threads, 1),
                                        kMaxStreams * PoolDevices(s.Device()).size()),
                       subimages_.size());
  // with a communicator each rank runs its own subimages on a pool of its own
  const size_t rank_workers =
      comm_ ? std::min<size_t>(n_workers, (subimages_.size() + comm_->Size() - 1) /
                                              size_t(comm_->Size()))
            : n_workers;
  if (rank_workers > 1) EnsureWorkers(s, rank_workers);
  Pass pass{data_image, model_image, result_model, psf_images, psf_indices,
            /*threshold=*/0.0, /*find_peak_only=*/true, /*pooled=*/rank_workers > 1};
  const double start_peak = RunPass(pass);
  log::Info() << "Maximum start peak over " << subimages_.size()
              << " subimages: " << start_peak << '\n';
  pass.threshold = start_peak * (1.0 - major_loop_gain);
  pass.find_peak_only = false;
  RunPass(pass);
  model_image.CopyFrom(result_model);

  ParallelDeconvolutionResult result;
  result.start_peak = float(start_peak);
  size_t finished = 0;
  bool reached_max = false;
  double end_peak = 0.0;
  for (const SubImage& sub : subimages_) {
    if (!sub.reached_major_threshold) ++finished;
    if (algorithms_[sub.index]->IterationNumber() >=
        algorithms_[sub.index]->MaxIterations())
      reached_max = true;
    end_peak = std::max(end_peak, sub.peak);
  }
  result.end_peak = float(end_peak);
  result.another_iteration_required = finished != subimages_.size() && !reached_max;
  log::Info() << finished << " / " << subimages_.size() << " sub-images finished\n";
  return result;
}

}  // namespace radler::algorithms
