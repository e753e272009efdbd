// A minimal FITS image reader and writer (no cfitsio): what Radler reads
// from disk — forced spectral-term cubes, clean masks, RMS images — and the
// horizon mask it writes (aocommon::FitsReader / FitsWriter in the
// reference, cpp/radler.cc:189-195, 410-527).
//
// Reader: the primary HDU only. 80-byte cards in 2880-byte blocks up to END;
// SIMPLE, BITPIX in {8, 16, 32, -32, -64}, NAXIS 2..4, NAXISn, BSCALE / BZERO
// and CTYPEn are honoured. Data are big-endian and converted to float.
// Pixel (x, y) of plane k is element k*w*h + y*w + x of the data in file
// order (no flip, as aocommon::FitsReader fills an Image). Every malformed
// input — a truncated file, no END card, NAXIS < 2, a negative or overflowing
// size, an unsupported BITPIX — throws std::runtime_error naming the file.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace radler {

class FitsImageReader {
 public:
  /// Parses the header. A file that cannot be opened throws
  /// "<what> '<path>' is not available: <strerror>" (`what` names the file's
  /// role in the message, e.g. "Forced spectrum file").
  explicit FitsImageReader(const std::string& path, const std::string& what = "FITS file");

  size_t Width() const { return width_; }
  size_t Height() const { return height_; }
  /// Product of NAXIS3.. (1 for a 2-D image).
  size_t NImages() const { return n_images_; }
  /// Length of the axis whose CTYPE starts with FREQ (1 when there is none).
  size_t NFrequencies() const { return n_frequencies_; }

  /// All NImages() planes (NImages() * Width() * Height() floats).
  void Read(float* data) const { ReadPlanes(data, 0, n_images_); }
  /// Plane `index` (Width() * Height() floats).
  void ReadIndex(float* data, size_t index) const;

 private:
  void ReadPlanes(float* data, size_t first, size_t count) const;
  [[noreturn]] void Fail(const std::string& why) const;

  std::string path_;
  size_t width_ = 0, height_ = 0, n_images_ = 1, n_frequencies_ = 1;
  int bitpix_ = 0;
  double bscale_ = 1.0, bzero_ = 0.0;
  uint64_t data_offset_ = 0, file_size_ = 0;
};

/// A 2-D float image: SIMPLE, BITPIX = -32, NAXIS = 2, NAXIS1/2, CDELT1 =
/// -pixel_scale_x and CDELT2 = pixel_scale_y in degrees (the scales are in
/// radians), END, big-endian data padded to a 2880-byte block.
void WriteFitsImage(const std::string& path, const float* data, size_t width,
                    size_t height, double pixel_scale_x, double pixel_scale_y);

}  // namespace radler
