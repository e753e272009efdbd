// Minimal stand-ins for the aocommon / schaapcommon types that Radler's
// public headers use (cpp/settings.h, work_table_entry.h, radler.h). The
// reference takes them from the external/aocommon and external/schaapcommon
// submodules (empty in the snapshot). When this library is built inside a
// project that already provides the real aocommon (WSClean), define
// RADLER_AMD_USE_EXTERNAL_AOCOMMON and these definitions are skipped.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#ifndef RADLER_AMD_USE_EXTERNAL_AOCOMMON
namespace aocommon {

// Values follow aocommon/polarization.h (FITS / casacore codes).
enum PolarizationEnum {
  StokesI = 1,
  StokesQ = 2,
  StokesU = 3,
  StokesV = 4,
  RR = -1,
  LL = -2,
  RL = -3,
  LR = -4,
  XX = -5,
  YY = -6,
  XY = -7,
  YX = -8,
  FullStokes = 10,
  DiagonalInstrumental = 11,
  Instrumental = 12,
  Diagonal = 13
};

struct Polarization {
  static bool IsStokes(PolarizationEnum p) {
    return p == StokesI || p == StokesQ || p == StokesU || p == StokesV;
  }
  static bool HasDualPolarization(const std::set<PolarizationEnum>& p) {
    return (p.count(XX) && p.count(YY)) || (p.count(RR) && p.count(LL));
  }
  static bool HasFullLinearPolarization(const std::set<PolarizationEnum>& p) {
    return p.count(XX) && p.count(XY) && p.count(YX) && p.count(YY);
  }
  static bool HasFullCircularPolarization(const std::set<PolarizationEnum>& p) {
    return p.count(RR) && p.count(RL) && p.count(LR) && p.count(LL);
  }
  static std::string TypeToShortString(PolarizationEnum p) {
    switch (p) {
      case StokesI: return "I";
      case StokesQ: return "Q";
      case StokesU: return "U";
      case StokesV: return "V";
      case RR: return "RR";
      case LL: return "LL";
      case RL: return "RL";
      case LR: return "LR";
      case XX: return "XX";
      case YY: return "YY";
      case XY: return "XY";
      case YX: return "YX";
      default: return "?";
    }
  }
};

namespace system {
inline size_t ProcessorCount() {
  const unsigned n = std::thread::hardware_concurrency();
  return n == 0 ? 1 : n;
}
}  // namespace system

// A row-major float image, owning or viewing (aocommon::Image subset).
class Image {
 public:
  Image() = default;
  Image(size_t width, size_t height)
      : width_(width), height_(height), owned_(width * height) {
    data_ = owned_.data();
  }
  Image(size_t width, size_t height, float value)
      : width_(width), height_(height), owned_(width * height, value) {
    data_ = owned_.data();
  }
  // Non-owning view (aocommon::Image(float*, w, h)).
  Image(float* data, size_t width, size_t height)
      : width_(width), height_(height), data_(data) {}
  Image(const Image& o) : width_(o.width_), height_(o.height_) {
    owned_.assign(o.data_, o.data_ + o.Size());
    data_ = owned_.data();
  }
  Image(Image&& o) noexcept { *this = std::move(o); }
  Image& operator=(const Image& o) {
    if (this != &o) {
      width_ = o.width_;
      height_ = o.height_;
      owned_.assign(o.data_, o.data_ + o.Size());
      data_ = owned_.data();
    }
    return *this;
  }
  Image& operator=(Image&& o) noexcept {
    width_ = o.width_;
    height_ = o.height_;
    const bool owns = o.data_ == o.owned_.data() && !o.owned_.empty();
    owned_ = std::move(o.owned_);
    data_ = owns ? owned_.data() : o.data_;
    o.data_ = nullptr;
    o.width_ = o.height_ = 0;
    return *this;
  }
  Image& operator=(float v) {
    std::fill_n(data_, Size(), v);
    return *this;
  }
  size_t Width() const { return width_; }
  size_t Height() const { return height_; }
  size_t Size() const { return width_ * height_; }
  bool Empty() const { return Size() == 0; }
  float* Data() { return data_; }
  const float* Data() const { return data_; }
  float& operator[](size_t i) { return data_[i]; }
  const float& operator[](size_t i) const { return data_[i]; }
  float* begin() { return data_; }
  float* end() { return data_ + Size(); }
  const float* begin() const { return data_; }
  const float* end() const { return data_ + Size(); }
  void Reset() {
    owned_.clear();
    owned_.shrink_to_fit();
    data_ = nullptr;
    width_ = height_ = 0;
  }

 private:
  size_t width_ = 0, height_ = 0;
  std::vector<float> owned_;
  float* data_ = nullptr;
};

// aocommon/imageaccessor.h
class ImageAccessor {
 public:
  virtual ~ImageAccessor() = default;
  virtual size_t Width() const = 0;
  virtual size_t Height() const = 0;
  virtual void Load(float* data) const = 0;
  virtual void Store(const float* data) = 0;
};

// aocommon/imagecoordinates.h: the direction cosines of pixel (x, y); l
// grows to the left of the image centre, m upwards
struct ImageCoordinates {
  template <typename T>
  static void XYToLM(size_t x, size_t y, T pixel_size_x, T pixel_size_y, size_t width,
                     size_t height, T& l, T& m) {
    const T mid_x = T(width) / T(2), mid_y = T(height) / T(2);
    l = (mid_x - T(x)) * pixel_size_x;
    m = (T(y) - mid_y) * pixel_size_y;
  }
  // the direction (l, m) seen from phase centre (ra0, dec0)
  template <typename T>
  static void LMToRaDec(T l, T m, T phase_centre_ra, T phase_centre_dec, T& ra, T& dec) {
    const T n = std::sqrt(T(1) - l * l - m * m);
    const T cos_dec0 = std::cos(phase_centre_dec), sin_dec0 = std::sin(phase_centre_dec);
    ra = phase_centre_ra + std::atan2(l, n * cos_dec0 - m * sin_dec0);
    dec = std::asin(m * cos_dec0 + n * sin_dec0);
  }
  // the inverse of LMToRaDec: the direction cosines of (ra, dec). A direction
  // on the far hemisphere has the (l, m) of its mirror image: RaDecToN tells
  template <typename T>
  static void RaDecToLM(T ra, T dec, T phase_centre_ra, T phase_centre_dec, T& l, T& m) {
    const T delta = ra - phase_centre_ra;
    const T cos_dec = std::cos(dec), sin_dec = std::sin(dec);
    const T cos_dec0 = std::cos(phase_centre_dec), sin_dec0 = std::sin(phase_centre_dec);
    l = cos_dec * std::sin(delta);
    m = sin_dec * cos_dec0 - cos_dec * sin_dec0 * std::cos(delta);
  }
  // the third direction cosine, negative behind the phase centre
  template <typename T>
  static T RaDecToN(T ra, T dec, T phase_centre_ra, T phase_centre_dec) {
    return std::sin(dec) * std::sin(phase_centre_dec) +
           std::cos(dec) * std::cos(phase_centre_dec) * std::cos(ra - phase_centre_ra);
  }
  // the inverse of XYToLM, fractional: a direction between pixel centres
  template <typename T>
  static void LMToXY(T l, T m, T pixel_size_x, T pixel_size_y, size_t width, size_t height,
                     T& x, T& y) {
    const T mid_x = T(width) / T(2), mid_y = T(height) / T(2);
    x = mid_x - l / pixel_size_x;
    y = mid_y + m / pixel_size_y;
  }
};

// aocommon/radeccoord.h, the two formatters the source catalogue uses
// (restated from their published behaviour; parity unpinned — DESIGN.md)
struct RaDecCoord {
  /// HH:MM:SS.sss of fmod(ra, 24 h), rounded to 1/1000 s; a negative angle
  /// keeps its sign (it is not wrapped to 0..24 h)
  static std::string RAToString(long double ra, char delimiter) {
    constexpr long double kPi = 3.141592653589793238462643383279502884L;
    const long double hours = std::fmod(ra * (12.0L / kPi), 24.0L);
    return Sexagesimal(hours, delimiter);
  }
  /// DD.MM.SS.sss, rounded to 1/1000 arcsec; '-' when negative, no '+'
  static std::string DecToString(long double dec, char delimiter) {
    constexpr long double kPi = 3.141592653589793238462643383279502884L;
    return Sexagesimal(dec * (180.0L / kPi), delimiter);
  }

 private:
  static std::string Sexagesimal(long double units, char delimiter) {
    const long long parts = std::llround(std::fabs(units) * 3600000.0L);
    const long long whole = parts / 3600000, minutes = parts / 60000 % 60,
                    seconds = parts / 1000 % 60, milli = parts % 1000;
    std::string s;
    if (units < 0.0L && parts != 0) s += '-';
    if (whole < 10) s += '0';
    s += std::to_string(whole);
    s += delimiter;
    s += char('0' + minutes / 10);
    s += char('0' + minutes % 10);
    s += delimiter;
    s += char('0' + seconds / 10);
    s += char('0' + seconds % 10);
    s += '.';
    s += char('0' + milli / 100);
    s += char('0' + milli / 10 % 10);
    s += char('0' + milli % 10);
    return s;
  }
};

}  // namespace aocommon

namespace schaapcommon::fitters {
// schaapcommon/fitters/spectralfitter.h
enum class SpectralFittingMode {
  kNoFitting,
  kPolynomial,
  kLogPolynomial,
  kForcedTerms
};
}  // namespace schaapcommon::fitters
#endif  // RADLER_AMD_USE_EXTERNAL_AOCOMMON
