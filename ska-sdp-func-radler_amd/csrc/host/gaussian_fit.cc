// See gaussian_fit.h for the contracts and the Levenberg-Marquardt rules.
#include "gaussian_fit.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "host_profile.h"

namespace schaapcommon::fitters {

using math::Ellipse;
using radler::gpu::Session;

namespace {

constexpr int kParams = 6;

struct Box {
  uint32_t x, y, w, h;
};

// index of (i, j), i <= j, in the row-by-row upper triangle
inline int Tri(int i, int j) { return i * kParams - i * (i - 1) / 2 + (j - i); }

void Evaluate(Session& s, const float* d_image, size_t width, size_t height, const Box& box,
              const double* p, double* sums) {
  radler::gpu::Check(
      rdl_gaussian_fit_sums(s.Handle(), d_image, uint32_t(width), uint32_t(height), box.x, box.y,
                            box.w, box.h, p, sums),
      "rdl_gaussian_fit_sums");
}

// Gaussian elimination with partial pivoting; false when singular
bool Solve(int n, double a[kParams][kParams], double* b) {
  for (int c = 0; c < n; ++c) {
    int pivot = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(a[r][c]) > std::fabs(a[pivot][c])) pivot = r;
    if (!(std::fabs(a[pivot][c]) > 0.0) || !std::isfinite(a[pivot][c])) return false;
    if (pivot != c) {
      for (int k = 0; k < n; ++k) std::swap(a[c][k], a[pivot][k]);
      std::swap(b[c], b[pivot]);
    }
    for (int r = c + 1; r < n; ++r) {
      const double f = a[r][c] / a[c][c];
      for (int k = c; k < n; ++k) a[r][k] -= f * a[c][k];
      b[r] -= f * b[c];
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double v = b[r];
    for (int k = r + 1; k < n; ++k) v -= a[r][k] * b[k];
    b[r] = v / a[r][r];
  }
  return true;
}

void Normalise(double* p) {
  if (p[4] > p[3]) {
    std::swap(p[3], p[4]);
    p[5] += M_PI_2;
  }
  p[5] -= M_PI * std::floor(p[5] / M_PI + 0.5);
}

void LevenbergMarquardt(Session& s, const float* d_image, size_t width, size_t height,
                        const Box& box, double* p, const bool* is_free) {
  double sums[RDL_GAUSSIAN_FIT_SUMS], trial_sums[RDL_GAUSSIAN_FIT_SUMS];
  Evaluate(s, d_image, width, height, box, p, sums);
  size_t evaluations = 1;
  double lambda = kLmLambdaStart;
  while (evaluations < kLmMaxEvaluations) {
    int idx[kParams], n = 0;
    for (int i = 0; i < kParams; ++i)
      if (is_free[i] && sums[Tri(i, i)] > 0.0) idx[n++] = i;
    if (n == 0) break;
    double a[kParams][kParams], delta[kParams];
    for (int r = 0; r < n; ++r) {
      for (int c = 0; c < n; ++c)
        a[r][c] = sums[Tri(std::min(idx[r], idx[c]), std::max(idx[r], idx[c]))];
      a[r][r] *= 1.0 + lambda;
      delta[r] = sums[21 + idx[r]];
    }
    bool accepted = false;
    double trial[kParams];
    if (Solve(n, a, delta)) {
      for (int i = 0; i < kParams; ++i) trial[i] = p[i];
      for (int r = 0; r < n; ++r) trial[idx[r]] += delta[r];
      bool valid = trial[3] > 0.0 && trial[4] > 0.0;
      for (int i = 0; i < kParams; ++i) valid = valid && std::isfinite(trial[i]);
      if (valid) {
        Evaluate(s, d_image, width, height, box, trial, trial_sums);
        ++evaluations;
        accepted = trial_sums[27] < sums[27];
      }
    }
    if (accepted) {
      double step = 0.0;
      for (int r = 0; r < n; ++r)
        step = std::max(step, std::fabs(delta[r]) / std::max(std::fabs(trial[idx[r]]), 1.0));
      const bool done = step < kLmStepTolerance ||
                        sums[27] - trial_sums[27] <= kLmDecreaseTolerance * sums[27];
      std::copy_n(trial, kParams, p);
      std::copy_n(trial_sums, RDL_GAUSSIAN_FIT_SUMS, sums);
      lambda = std::max(lambda / 10.0, kLmLambdaMin);
      if (done) break;
    } else {
      lambda *= 10.0;
      if (lambda > kLmLambdaMax) break;
    }
  }
  Normalise(p);
}

size_t BoxSide(double major) {
  double side = std::max(10.0, std::ceil(10.0 * major));
  if (!(side < 1e9)) side = 1e9;  // also a non-finite major
  size_t n = size_t(side);
  if (n & 1) ++n;
  return n;
}

// the box rule of Fit2DGaussianFull; false when the box misses the image
bool MakeBox(size_t width, size_t height, size_t side, double x, double y, Box& box,
             bool& whole) {
  whole = side >= width && side >= height;
  if (whole) {
    box = Box{0, 0, uint32_t(width), uint32_t(height)};
    return true;
  }
  if (!std::isfinite(x) || !std::isfinite(y) || std::fabs(x) > 1e9 || std::fabs(y) > 1e9)
    return false;
  const long long half = (long long)(side / 2);
  const long long x0 = std::llround(x) - half, y0 = std::llround(y) - half;
  const long long xa = std::clamp<long long>(x0, 0, (long long)width);
  const long long xb = std::clamp<long long>(x0 + (long long)side, 0, (long long)width);
  const long long ya = std::clamp<long long>(y0, 0, (long long)height);
  const long long yb = std::clamp<long long>(y0 + (long long)side, 0, (long long)height);
  if (xb <= xa || yb <= ya) return false;
  box = Box{uint32_t(xa), uint32_t(ya), uint32_t(xb - xa), uint32_t(yb - ya)};
  return true;
}

void FitRounds(Session& s, const float* d_image, size_t width, size_t height, double* p,
               const bool* is_free) {
  size_t side = BoxSide(p[3]);
  for (size_t round = 0; round != kFitMaxRounds; ++round) {
    Box box;
    bool whole;
    if (!MakeBox(width, height, side, p[1], p[2], box, whole)) break;
    LevenbergMarquardt(s, d_image, width, height, box, p, is_free);
    if (whole) break;
    const size_t new_side = BoxSide(p[3]);
    if (new_side == side) break;
    side = new_side;
  }
}

}  // namespace

void Fit2DGaussianFull(Session& s, const float* d_image, size_t width, size_t height,
                       double& amplitude, double& x, double& y, double& major, double& minor,
                       double& position_angle) {
  radler::prof::Section prof_section("fit.gaussian_full");
  double p[kParams] = {amplitude, x, y, major, minor, position_angle};
  const bool is_free[kParams] = {true, true, true, true, true, true};
  if (!(p[3] > 0.0) || !(p[4] > 0.0)) return;
  FitRounds(s, d_image, width, height, p, is_free);
  amplitude = p[0];
  x = p[1];
  y = p[2];
  major = p[3];
  minor = p[4];
  position_angle = p[5];
}

Ellipse Fit2DGaussianCentred(Session& s, const float* d_image, size_t width, size_t height,
                             double beam_estimate) {
  radler::prof::Section prof_section("fit.gaussian_centred");
  if (!(beam_estimate > 0.0)) beam_estimate = 1.0;
  const size_t cx = width / 2, cy = height / 2;
  const double centre = s.ReadFloat(d_image + cx + cy * width);
  double p[kParams] = {centre, double(cx), double(cy), beam_estimate, beam_estimate, 0.0};
  const bool is_free[kParams] = {false, false, false, true, true, true};
  if (std::isfinite(centre)) FitRounds(s, d_image, width, height, p, is_free);
  return Ellipse{p[3], p[4], p[5]};
}

Ellipse DeconvolveGaussian(const Ellipse& ellipse, const Ellipse& psf) {
  // second moments (in FWHM^2 units): R diag(major^2, minor^2) R^T
  auto moments = [](const Ellipse& e, double& xx, double& xy, double& yy) {
    const double a = e.major * e.major, b = e.minor * e.minor;
    const double cs = std::cos(e.position_angle), sn = std::sin(e.position_angle);
    xx = a * cs * cs + b * sn * sn;
    xy = (a - b) * cs * sn;
    yy = a * sn * sn + b * cs * cs;
  };
  double exx, exy, eyy, pxx, pxy, pyy;
  moments(ellipse, exx, exy, eyy);
  moments(psf, pxx, pxy, pyy);
  const double xx = exx - pxx, xy = exy - pxy, yy = eyy - pyy;
  const double trace = xx + yy, diff = xx - yy;
  const double root = std::sqrt(diff * diff + 4.0 * xy * xy);
  const double l1 = 0.5 * (trace + root), l2 = 0.5 * (trace - root);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (!(l2 > 0.0) || !std::isfinite(l1)) return Ellipse{nan, nan, nan};
  Ellipse out;
  out.major = std::sqrt(l1);
  out.minor = std::sqrt(l2);
  out.position_angle = root > 0.0 ? 0.5 * std::atan2(2.0 * xy, diff) : 0.0;
  return out;
}

}  // namespace schaapcommon::fitters
