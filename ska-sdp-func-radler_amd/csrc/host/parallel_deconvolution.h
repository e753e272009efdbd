// radler::algorithms::ParallelDeconvolution (reference:
// cpp/algorithms/parallel_deconvolution.{h,cc}). One subimage runs the
// algorithm on the whole device-resident image set; a grid splits the image
// into subimages (Dijkstra minimum-flux boundaries), finds the global start
// peak, and deconvolves every subimage on the device.
#pragma once

#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <vector>

#include "communicator.h"
#include "component_list.h"
#include "deconvolution_algorithm.h"
#include "device.h"
#include "psf_offset.h"
#include "settings.h"
#include "subimage_split.h"

namespace radler::algorithms {

struct ParallelDeconvolutionResult {
  bool another_iteration_required = false;
  std::optional<float> start_peak;
  std::optional<float> end_peak;
};

class ParallelDeconvolution {
 public:
  explicit ParallelDeconvolution(const Settings& settings);
  ~ParallelDeconvolution();

  DeconvolutionAlgorithm& FirstAlgorithm() { return *algorithms_.front(); }
  const DeconvolutionAlgorithm& FirstAlgorithm() const {
    return *algorithms_.front();
  }
  const DeconvolutionAlgorithm& MaxScaleCountAlgorithm() const;
  void SetAlgorithm(std::unique_ptr<DeconvolutionAlgorithm> algorithm);
  void SetThreshold(double threshold);
  void SetMinorLoopGain(double gain);
  void SetCleanMask(const bool* mask);
  /// GetComponentList for multiscale (parallel_deconvolution.cc:184-196);
  /// with a process-per-GPU split each rank holds its own subimages'.
  ComponentList GetMultiscaleComponentList() const;
  /// parallel_deconvolution.cc:271-276
  void SetComponentOptimization(OptimizationAlgorithm algorithm) {
    for (auto& a : algorithms_) a->SetComponentOptimizationAlgorithm(algorithm);
  }
  /// parallel_deconvolution.cc:244-250: the single algorithm takes it as
  /// is; gridded runs trim each subimage's box (:332-337) and drop it after
  /// the run (:421-423). nullptr clears it.
  void SetRmsFactorImage(std::shared_ptr<const std::vector<float>> image, size_t width);
  /// parallel_deconvolution.cc:285-292: the term planes of a kForcedTerms
  /// fitter (NTerms() - 1 full-image planes, rows of `width` floats). The
  /// single algorithm takes them as they are; in gridded runs every
  /// subimage's algorithm gets the same full planes with its own origin
  /// (where the reference trims a copy per subimage, :340-349).
  void SetSpectrallyForcedImages(std::vector<std::vector<float>> planes, size_t width);
  /// Auto-masking (parallel_deconvolution.cc:260-268): passed to the
  /// multiscale algorithms; gridded runs keep full-image per-scale masks and
  /// hand each subimage its box (:359-390), merging it back inside the
  /// boundary mask after a converging run (:425-462).
  void SetAutoMaskMode(bool track_per_scale_masks, bool use_per_scale_masks);
  bool IsInitialized() const { return !algorithms_.empty(); }
  size_t SubImageCount() const { return algorithms_.size(); }
  DeconvolutionAlgorithm& Algorithm(size_t i) { return *algorithms_[i]; }
  const DeconvolutionAlgorithm& Algorithm(size_t i) const { return *algorithms_[i]; }

  ParallelDeconvolutionResult ExecuteMajorIteration(
      ImageSet& data_image, ImageSet& model_image,
      const std::vector<gpu::Planes>& psf_images,
      const std::vector<PsfOffset>& psf_offsets, double major_loop_gain);

  /// Tiles of the last ExecuteParallelRun (empty for a 1x1 grid).
  const std::vector<SubImage>& SubImages() const { return subimages_; }
  /// Process-per-GPU: the rank that cleaned each subimage in the last major
  /// iteration (empty without a communicator).
  const std::vector<int>& CleanOwners() const { return clean_owners_; }

  void FreeDeconvolutionAlgorithms() {
    algorithms_.clear();
    workers_.clear();
    worker_main_device_ = -1;
    mask_ = nullptr;
    forced_images_.reset();
  }
  /// Share the subimages of gridded runs with the other ranks of a
  /// process-per-GPU job (a size-1 communicator runs them all here, in the
  /// same snapshot order). Every rank must call Perform with the same inputs.
  void SetCommunicator(std::shared_ptr<Communicator> comm) { comm_ = std::move(comm); }
  const std::shared_ptr<Communicator>& GetCommunicator() const { return comm_; }
  /// Worker streams of the concurrent subimage pool (0 until a gridded run
  /// with settings.parallel.max_threads > 1).
  size_t WorkerCount() const { return workers_.size(); }

 private:
  ParallelDeconvolutionResult ExecuteSingleThreadedRun(
      ImageSet& data_image, ImageSet& model_image,
      const std::vector<gpu::Planes>& psf_images,
      const std::vector<PsfOffset>& psf_offsets, double major_loop_gain);
  ParallelDeconvolutionResult ExecuteParallelRun(
      ImageSet& data_image, ImageSet& model_image,
      const std::vector<gpu::Planes>& psf_images,
      const std::vector<PsfOffset>& psf_offsets, double major_loop_gain);

  struct Pass;         // what one pass over the subimages works on
  struct SubImageRun;  // one subimage's device planes through a pass
  /// Per-subimage result of a snapshot pass (device planes on the main
  /// device, valid during the call): the residual box, the model box to add
  /// (the initial one when it diverged) and whether it converged.
  using SubImageSink = std::function<void(size_t index, const float* d_data,
                                          const float* d_model, bool converging)>;

  /// Sequential, pool or distributed; returns the start peak.
  double RunPass(const Pass& pass);
  /// Runs the algorithm of `sub`; returns whether it converged.
  bool DeconvolveSubImage(SubImage& sub, ImageSet& sub_data, ImageSet& sub_model,
                          const gpu::Planes& sub_psfs, double major_iteration_threshold,
                          bool find_peak_only);
  /// The subimages (those with run[i] != 0, given `run`) one after another on
  /// the calling thread. Without a sink each is merged at once and the next sees
  /// it (the reference with one thread); with one, all see the pass-start residual.
  void RunSubImagesInTurn(const Pass& pass, const std::vector<char>* run = nullptr,
                          const SubImageSink& sink = nullptr);
  /// The same on the worker pool, every one from the pass-start residual; the
  /// results are merged, or handed to `sink`, in subimage order.
  void RunSubImagesConcurrently(const Pass& pass, const std::vector<char>* run = nullptr,
                                const SubImageSink& sink = nullptr);
  /// Process-per-GPU split; returns the global start peak (find-peak pass).
  double RunSubImagesDistributed(const Pass& pass);
  void EnsureWorkers(gpu::Session& main, size_t n);
  /// the subimage's box of the full-image scale masks into its algorithm
  void LoadScaleMasks(const SubImage& sub, size_t width);
  /// the algorithm's scale masks of `sub` (subimage-sized, one per scale)
  std::vector<std::vector<uint8_t>> SubImageScaleMasks(const SubImage& sub);
  /// merge subimage-sized scale masks into the full-image ones (boundary mask)
  void StoreScaleMasks(const SubImage& sub, size_t width, size_t height,
                       const std::vector<std::vector<uint8_t>>& sub_masks);
  static std::vector<int> PoolDevices(int main_device);

  // worker sessions (one stream each) outlive the algorithms, whose cached
  // transforms and scratch live on them
  std::vector<std::shared_ptr<gpu::Session>> workers_;
  // process-per-GPU: the cleaning pass's subimage owners (LptOwners over the
  // find-peak pass's estimates), identical on every rank
  std::vector<int> clean_owners_;
  int worker_main_device_ = -1;
  std::vector<std::unique_ptr<DeconvolutionAlgorithm>> algorithms_;
  std::vector<SubImage> subimages_;
  const Settings& settings_;
  const bool* mask_ = nullptr;
  std::shared_ptr<const std::vector<float>> rms_image_;  // full image (gridded)
  std::shared_ptr<const ForcedTermImages> forced_images_;  // full image (gridded)
  std::unique_ptr<ComponentList> component_list_;        // gridded multiscale
  size_t rms_width_ = 0;
  std::shared_ptr<Communicator> comm_;
  bool track_masks_ = false, use_masks_ = false;
  std::vector<std::vector<uint8_t>> scale_masks_;  // full image, per scale
  std::mutex masks_mutex_;
};

/// A subimage's work in a pass, for the pool's queue and the ranks' LptOwners:
/// cleaning grows with the area and with how far the peak lies above the threshold
/// (components ~ log(peak / threshold) per source at a fixed gain); finding, with area.
double SubImageCost(size_t area, double peak, double threshold, bool find_peak_only);

/// How the pool's workers share the subimages of a pass.
struct PoolAssignment {
  std::vector<size_t> order;    // the subimages in the order they are taken
  bool shared_counter = false;  // a free worker takes order[next++]; else w: w, w + W, ...
  std::vector<char> staged;     // per subimage: trimmed on the main device, peer-copied
};

/// For `queue_mode` (RADLER_POOL_QUEUE, see the definition) and the subimages with
/// run[i] != 0 (all without `run`), costs[i] each; worker_local[w]: on the main device.
PoolAssignment AssignPool(int queue_mode, const std::vector<char>& worker_local,
                          bool force_staging, const std::vector<double>& costs,
                          const std::vector<char>* run = nullptr);

}  // namespace radler::algorithms
