#include "fits_image.h"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>

namespace radler {
namespace {

constexpr size_t kCard = 80, kBlock = 2880;

struct FileCloser {
  void operator()(std::FILE* f) const {
    if (f) std::fclose(f);
  }
};
using File = std::unique_ptr<std::FILE, FileCloser>;

std::string Trimmed(const char* begin, const char* end) {
  while (begin != end && *begin == ' ') ++begin;
  while (end != begin && end[-1] == ' ') --end;
  return std::string(begin, end);
}

// The value field of a card (columns 11-80): a quoted string without its
// quotes, or the text before the comment's '/'.
std::string CardValue(const char* card) {
  const char* p = card + 10;
  const char* end = card + kCard;
  while (p != end && *p == ' ') ++p;
  if (p != end && *p == '\'') {
    const char* q = ++p;
    while (q != end && *q != '\'') ++q;
    return Trimmed(p, q);
  }
  const char* q = p;
  while (q != end && *q != '/') ++q;
  return Trimmed(p, q);
}

bool ParseInteger(const std::string& text, long long* out) {
  if (text.empty()) return false;
  errno = 0;
  char* end = nullptr;
  const long long v = std::strtoll(text.c_str(), &end, 10);
  if (errno != 0 || end == text.c_str() || *end != '\0') return false;
  *out = v;
  return true;
}

bool ParseReal(std::string text, double* out) {
  for (char& c : text)
    if (c == 'D' || c == 'd') c = 'E';  // Fortran exponent
  if (text.empty()) return false;
  errno = 0;
  char* end = nullptr;
  const double v = std::strtod(text.c_str(), &end);
  if (end == text.c_str() || *end != '\0' || !std::isfinite(v)) return false;
  *out = v;
  return true;
}

template <class T>
T BigEndian(const unsigned char* p) {
  uint64_t bits = 0;
  for (size_t i = 0; i != sizeof(T); ++i) bits = (bits << 8) | p[i];
  T v;
  if constexpr (sizeof(T) == 1) {
    const uint8_t b = uint8_t(bits);
    std::memcpy(&v, &b, 1);
  } else if constexpr (sizeof(T) == 2) {
    const uint16_t b = uint16_t(bits);
    std::memcpy(&v, &b, 2);
  } else if constexpr (sizeof(T) == 4) {
    const uint32_t b = uint32_t(bits);
    std::memcpy(&v, &b, 4);
  } else {
    std::memcpy(&v, &bits, 8);
  }
  return v;
}

}  // namespace

void FitsImageReader::Fail(const std::string& why) const {
  throw std::runtime_error("FITS file '" + path_ + "': " + why);
}

FitsImageReader::FitsImageReader(const std::string& path, const std::string& what)
    : path_(path) {
  File f(std::fopen(path.c_str(), "rb"));
  if (!f)
    throw std::runtime_error(what + " '" + path + "' is not available: " +
                             std::strerror(errno));
  if (std::fseek(f.get(), 0, SEEK_END) != 0) Fail("cannot seek");
  const long size = std::ftell(f.get());
  if (size < 0) Fail("cannot determine the file size");
  file_size_ = uint64_t(size);
  std::rewind(f.get());

  long long naxis = -1, axis[4] = {-1, -1, -1, -1};
  std::string ctype[4];
  bool have_bitpix = false, ended = false;
  uint64_t offset = 0;
  char card[kCard];
  while (!ended) {
    if (offset + kCard > file_size_ || std::fread(card, 1, kCard, f.get()) != kCard)
      Fail("the header has no END card within the file (truncated header)");
    offset += kCard;
    const std::string key = Trimmed(card, card + 8);
    if (offset == kCard) {
      if (key != "SIMPLE" || CardValue(card) != "T")
        Fail("not a standard FITS file (no SIMPLE = T)");
      continue;
    }
    if (key == "END") {
      ended = true;
      break;
    }
    if (card[8] != '=') continue;  // COMMENT, HISTORY, blank
    const std::string value = CardValue(card);
    long long iv = 0;
    if (key == "BITPIX") {
      if (!ParseInteger(value, &iv)) Fail("unreadable BITPIX");
      if (iv != 8 && iv != 16 && iv != 32 && iv != -32 && iv != -64)
        Fail("unsupported BITPIX " + value);
      bitpix_ = int(iv);
      have_bitpix = true;
    } else if (key == "NAXIS") {
      if (!ParseInteger(value, &iv)) Fail("unreadable NAXIS");
      if (iv < 2 || iv > 4)
        Fail("NAXIS = " + value + " is not supported (an image of 2 to 4 axes is required)");
      naxis = iv;
    } else if (key.size() == 6 && key.compare(0, 5, "NAXIS") == 0 && key[5] >= '1' &&
               key[5] <= '4') {
      if (!ParseInteger(value, &iv)) Fail("unreadable " + key);
      if (iv < 0) Fail("negative " + key);
      axis[key[5] - '1'] = iv;
    } else if (key.size() == 6 && key.compare(0, 5, "CTYPE") == 0 && key[5] >= '1' &&
               key[5] <= '4') {
      ctype[key[5] - '1'] = value;
    } else if (key == "BSCALE") {
      if (!ParseReal(value, &bscale_)) Fail("unreadable BSCALE");
    } else if (key == "BZERO") {
      if (!ParseReal(value, &bzero_)) Fail("unreadable BZERO");
    }
  }
  if (!have_bitpix) Fail("no BITPIX card");
  if (naxis < 0) Fail("no NAXIS card");
  // sizes: every axis present, the product within the file
  const uint64_t element = uint64_t(bitpix_ < 0 ? -bitpix_ : bitpix_) / 8;
  uint64_t count = 1;
  for (long long a = 0; a != naxis; ++a) {
    if (axis[a] < 0) Fail("no NAXIS" + std::to_string(a + 1) + " card");
    if (axis[a] == 0) Fail("empty image (NAXIS" + std::to_string(a + 1) + " = 0)");
    if (uint64_t(axis[a]) > (uint64_t(1) << 40) / count)
      Fail("the image size overflows");
    count *= uint64_t(axis[a]);
  }
  width_ = size_t(axis[0]);
  height_ = size_t(axis[1]);
  n_images_ = size_t(count / (uint64_t(axis[0]) * uint64_t(axis[1])));
  for (long long a = 2; a < naxis; ++a)
    if (ctype[a].compare(0, 4, "FREQ") == 0) n_frequencies_ = size_t(axis[a]);
  data_offset_ = (offset + kBlock - 1) / kBlock * kBlock;
  if (data_offset_ > file_size_ || count * element > file_size_ - data_offset_)
    Fail("truncated: the header describes " + std::to_string(count * element) +
         " bytes of data, the file holds " +
         std::to_string(file_size_ > data_offset_ ? file_size_ - data_offset_ : 0));
}

void FitsImageReader::ReadIndex(float* data, size_t index) const {
  if (index >= n_images_)
    Fail("image index " + std::to_string(index) + " out of range (" +
         std::to_string(n_images_) + " images)");
  ReadPlanes(data, index, 1);
}

void FitsImageReader::ReadPlanes(float* data, size_t first, size_t count) const {
  File f(std::fopen(path_.c_str(), "rb"));
  if (!f)
    throw std::runtime_error("FITS file '" + path_ + "' is not available: " +
                             std::strerror(errno));
  const size_t element = size_t(bitpix_ < 0 ? -bitpix_ : bitpix_) / 8;
  const uint64_t plane = uint64_t(width_) * height_;
  const uint64_t start = data_offset_ + uint64_t(first) * plane * element;
  if (std::fseek(f.get(), long(start), SEEK_SET) != 0) Fail("cannot seek to the data");
  const bool scaled = bscale_ != 1.0 || bzero_ != 0.0;
  std::vector<unsigned char> buffer(std::min<uint64_t>(plane * count, 1 << 16) * element);
  uint64_t done = 0;
  const uint64_t total = plane * count;
  while (done != total) {
    const size_t n = size_t(std::min<uint64_t>(total - done, buffer.size() / element));
    if (std::fread(buffer.data(), element, n, f.get()) != n)
      Fail("truncated: the data ended early");
    for (size_t i = 0; i != n; ++i) {
      const unsigned char* p = buffer.data() + i * element;
      double v = 0.0;
      switch (bitpix_) {
        case 8: v = double(*p); break;
        case 16: v = double(BigEndian<int16_t>(p)); break;
        case 32: v = double(BigEndian<int32_t>(p)); break;
        case -32: v = double(BigEndian<float>(p)); break;
        case -64: v = BigEndian<double>(p); break;
      }
      data[done + i] = float(scaled ? bzero_ + bscale_ * v : v);
    }
    done += n;
  }
}

void WriteFitsImage(const std::string& path, const float* data, size_t width,
                    size_t height, double pixel_scale_x, double pixel_scale_y) {
  std::string header;
  auto card = [&header](const std::string& text) {
    std::string c = text;
    c.resize(kCard, ' ');
    header += c;
  };
  auto keyword = [&card](const char* key, const std::string& value) {
    char line[kCard + 1];
    std::snprintf(line, sizeof line, "%-8s= %20s", key, value.c_str());
    card(line);
  };
  auto real = [](double v) {
    char text[32];
    std::snprintf(text, sizeof text, "%.13E", v);
    return std::string(text);
  };
  constexpr double kDegrees = 180.0 / 3.14159265358979323846;
  keyword("SIMPLE", "T");
  keyword("BITPIX", "-32");
  keyword("NAXIS", "2");
  keyword("NAXIS1", std::to_string(width));
  keyword("NAXIS2", std::to_string(height));
  keyword("CDELT1", real(-pixel_scale_x * kDegrees));
  keyword("CDELT2", real(pixel_scale_y * kDegrees));
  card("END");
  header.resize((header.size() + kBlock - 1) / kBlock * kBlock, ' ');

  const size_t n = width * height;
  std::vector<unsigned char> bytes((n * 4 + kBlock - 1) / kBlock * kBlock, 0);
  for (size_t i = 0; i != n; ++i) {
    uint32_t bits;
    std::memcpy(&bits, &data[i], 4);
    bytes[4 * i] = uint8_t(bits >> 24);
    bytes[4 * i + 1] = uint8_t(bits >> 16);
    bytes[4 * i + 2] = uint8_t(bits >> 8);
    bytes[4 * i + 3] = uint8_t(bits);
  }
  File f(std::fopen(path.c_str(), "wb"));
  if (!f)
    throw std::runtime_error("Cannot write FITS file '" + path + "': " + std::strerror(errno));
  if (std::fwrite(header.data(), 1, header.size(), f.get()) != header.size() ||
      std::fwrite(bytes.data(), 1, bytes.size(), f.get()) != bytes.size() ||
      std::fflush(f.get()) != 0)
    throw std::runtime_error("Cannot write FITS file '" + path + "': " + std::strerror(errno));
}

}  // namespace radler
