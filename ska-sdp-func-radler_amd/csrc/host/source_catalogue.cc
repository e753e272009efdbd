#include "source_catalogue.h"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <stdexcept>

#include "logger.h"
#include "logpoly.h"

namespace radler {

namespace {

constexpr long double kPi = 3.141592653589793238462643383279502884L;
constexpr long double kArcsec = kPi / (180.0L * 3600.0L);

std::string Trim(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a != b && std::isspace(static_cast<unsigned char>(s[a]))) ++a;
  while (b != a && std::isspace(static_cast<unsigned char>(s[b - 1]))) --b;
  return s.substr(a, b - a);
}

std::string Lower(std::string s) {
  for (char& c : s) c = char(std::tolower(static_cast<unsigned char>(c)));
  return s;
}

// One file being parsed: every error names it and the line.
struct Parser {
  std::string filename;
  size_t line = 0;

  [[noreturn]] void Fail(const std::string& why) const {
    throw std::runtime_error("Source catalogue '" + filename + "', line " +
                             std::to_string(line) + ": " + why);
  }

  // fields separated by commas that are not inside [...], trimmed
  std::vector<std::string> Split(const std::string& text) const {
    std::vector<std::string> fields;
    std::string field;
    int depth = 0;
    for (char c : text) {
      if (c == '[') {
        if (depth != 0) Fail("nested '['");
        ++depth;
      } else if (c == ']') {
        if (depth == 0) Fail("']' without '['");
        --depth;
      }
      if (c == ',' && depth == 0) {
        fields.push_back(Trim(field));
        field.clear();
      } else {
        field += c;
      }
    }
    if (depth != 0) Fail("unterminated '['");
    fields.push_back(Trim(field));
    return fields;
  }

  double Number(const std::string& text, const char* what) const {
    if (text.empty()) Fail(std::string("empty ") + what);
    errno = 0;
    char* end = nullptr;
    const double v = std::strtod(text.c_str(), &end);
    if (end != text.c_str() + text.size() || !std::isfinite(v))
      Fail(std::string("bad ") + what + " '" + text + "'");
    return v;
  }

  float Float(const std::string& text, const char* what) const {
    if (text.empty()) Fail(std::string("empty ") + what);
    char* end = nullptr;
    const float v = std::strtof(text.c_str(), &end);
    if (end != text.c_str() + text.size() || !std::isfinite(v))
      Fail(std::string("bad ") + what + " '" + text + "'");
    return v;
  }

  // digits only, as an integer
  long Whole(const std::string& text, const std::string& field, const char* what) const {
    if (text.empty() || text.size() > 9 ||
        !std::all_of(text.begin(), text.end(),
                     [](char c) { return std::isdigit(static_cast<unsigned char>(c)); }))
      Fail(std::string("bad ") + what + " '" + field + "'");
    return std::strtol(text.c_str(), nullptr, 10);
  }

  // [sign]A<d>B<d>C[.fff] -> sign (A + B / 60 + C.fff / 3600); the inverse of
  // RaDecCoord's formatter with delimiter d. With d == '.', the fraction of
  // the seconds is a fourth part.
  long double Sexagesimal(const std::string& field, char delimiter, bool allow_plus,
                          const char* what) const {
    std::string body = field;
    long double sign = 1.0L;
    if (!body.empty() && (body[0] == '-' || (allow_plus && body[0] == '+'))) {
      if (body[0] == '-') sign = -1.0L;
      body.erase(0, 1);
    }
    std::vector<std::string> parts;
    std::string part;
    for (char c : body) {
      if (c == delimiter) {
        parts.push_back(part);
        part.clear();
      } else {
        part += c;
      }
    }
    parts.push_back(part);
    std::string seconds;
    if (delimiter == '.') {
      if (parts.size() != 3 && parts.size() != 4)
        Fail(std::string("bad ") + what + " '" + field + "'");
      seconds = parts[2];
      if (parts.size() == 4) {
        Whole(parts[3], field, what);
        seconds += "." + parts[3];
      }
    } else {
      if (parts.size() != 3) Fail(std::string("bad ") + what + " '" + field + "'");
      seconds = parts[2];
      const size_t dot = seconds.find('.');
      if (dot != std::string::npos) {
        if (dot + 1 != seconds.size()) Whole(seconds.substr(dot + 1), field, what);
        Whole(seconds.substr(0, dot), field, what);
      }
    }
    if (seconds.find('.') == std::string::npos) Whole(seconds, field, what);
    const long whole = Whole(parts[0], field, what), minutes = Whole(parts[1], field, what);
    const long double sec = std::strtold(seconds.c_str(), nullptr);
    if (minutes >= 60 || !(sec < 60.0L)) Fail(std::string("bad ") + what + " '" + field + "'");
    return sign * ((long double)(whole) + (long double)(minutes) / 60.0L + sec / 3600.0L);
  }

  bool Boolean(const std::string& text) const {
    const std::string v = Lower(text);
    if (v == "true" || v == "1") return true;
    if (v == "false" || v == "0") return false;
    Fail("bad LogarithmicSI '" + text + "'");
  }

  // "[a, b, ...]", or one bare number
  std::vector<float> Terms(const std::string& text) const {
    std::vector<float> terms;
    if (text.empty()) return terms;
    if (text.front() != '[') {
      terms.push_back(Float(text, "spectral term"));
      return terms;
    }
    if (text.back() != ']') Fail("bad SpectralIndex '" + text + "'");
    const std::string inner = Trim(text.substr(1, text.size() - 2));
    if (inner.empty()) return terms;
    size_t start = 0;
    while (true) {
      const size_t comma = inner.find(',', start);
      terms.push_back(Float(Trim(inner.substr(start, comma - start)), "spectral term"));
      if (comma == std::string::npos) break;
      start = comma + 1;
    }
    return terms;
  }
};

enum Column {
  kName,
  kType,
  kRa,
  kDec,
  kI,
  kSpectralIndex,
  kLogarithmicSI,
  kReferenceFrequency,
  kMajorAxis,
  kMinorAxis,
  kOrientation,
  kColumnCount
};
const char* const kColumnNames[kColumnCount] = {
    "name",          "type",          "ra",
    "dec",           "i",             "spectralindex",
    "logarithmicsi", "referencefrequency", "majoraxis",
    "minoraxis",     "orientation"};

struct Header {
  std::vector<int> column_of_field;  // a Column, or -1 for an unknown column
  int field_of[kColumnCount];
  std::string default_of[kColumnCount];
};

// "Format = Name, Type, ..., ReferenceFrequency='1.5e8', ..."
bool ParseHeader(const Parser& p, const std::string& text, Header& header) {
  if (Lower(text.substr(0, 6)) != "format") return false;
  const std::string rest = Trim(text.substr(6));
  if (rest.empty() || rest[0] != '=') return false;
  std::fill_n(header.field_of, int(kColumnCount), -1);
  const std::vector<std::string> fields = p.Split(rest.substr(1));
  for (size_t f = 0; f != fields.size(); ++f) {
    std::string name = fields[f], value;
    const size_t eq = name.find('=');
    if (eq != std::string::npos) {
      value = Trim(name.substr(eq + 1));
      name = Trim(name.substr(0, eq));
      if (value.size() >= 2 && (value.front() == '\'' || value.front() == '"') &&
          value.back() == value.front())
        value = Trim(value.substr(1, value.size() - 2));
    }
    if (name.empty()) p.Fail("empty column name in the Format line");
    int column = -1;
    for (int c = 0; c != kColumnCount; ++c)
      if (Lower(name) == kColumnNames[c]) column = c;
    header.column_of_field.push_back(column);
    if (column < 0) continue;
    if (header.field_of[column] >= 0) p.Fail("column '" + name + "' is listed twice");
    header.field_of[column] = int(f);
    header.default_of[column] = value;
  }
  for (int c : {kName, kType, kRa, kDec, kI})
    if (header.field_of[c] < 0)
      p.Fail(std::string("the Format line has no '") + kColumnNames[c] + "' column");
  return true;
}

struct Covariance {
  long double xx = 0.0L, xy = 0.0L, yy = 0.0L;
  long double Det() const { return xx * yy - xy * xy; }
};

// An elliptical Gaussian (sigmas in radians, position angle as beam_pa in
// restore.h: the major axis along (cos, sin)(pa + pi/2) in (l, m)) as a
// covariance in pixels, through J = diag(-1/pixel_scale_x, 1/pixel_scale_y)
Covariance PixelCovariance(long double sigma_major, long double sigma_minor, long double pa,
                           long double pixel_scale_x, long double pixel_scale_y) {
  const long double angle = pa + 0.5L * kPi;
  const long double ca = cosl(angle), sa = sinl(angle);
  const long double a = sigma_major * sigma_major, b = sigma_minor * sigma_minor;
  const long double ll = a * ca * ca + b * sa * sa;
  const long double lm = (a - b) * ca * sa;
  const long double mm = a * sa * sa + b * ca * ca;
  return {ll / (pixel_scale_x * pixel_scale_x), -lm / (pixel_scale_x * pixel_scale_y),
          mm / (pixel_scale_y * pixel_scale_y)};
}

long double FwhmToSigma() { return 1.0L / (2.0L * sqrtl(2.0L * logl(2.0L))); }

}  // namespace

SourceCatalogue SourceCatalogue::Read(const std::string& filename) {
  std::ifstream file(filename);
  if (!file)
    throw std::runtime_error("Source catalogue '" + filename +
                             "' is not available: " + std::strerror(errno));
  SourceCatalogue catalogue;
  Parser p{filename, 0};
  Header header;
  bool have_header = false;
  std::string raw;
  while (std::getline(file, raw)) {
    ++p.line;
    const std::string text = Trim(raw);
    if (text.empty() || text[0] == '#') continue;
    if (!have_header) {
      if (!ParseHeader(p, text, header))
        p.Fail("expected the 'Format = ...' line before the first source");
      have_header = true;
      const std::string& reference = header.default_of[kReferenceFrequency];
      if (!reference.empty()) {
        catalogue.header_reference_frequency_ = p.Number(reference, "ReferenceFrequency");
        if (!(catalogue.header_reference_frequency_ > 0.0))
          p.Fail("the default ReferenceFrequency is not positive");
      }
      continue;
    }
    const std::vector<std::string> fields = p.Split(text);
    if (fields.size() > header.column_of_field.size())
      p.Fail(std::to_string(fields.size()) + " fields for " +
             std::to_string(header.column_of_field.size()) + " columns");
    // a field, the column's default when it is empty or (optional columns
    // only) missing at the end of the row
    auto field = [&](Column c) -> std::string {
      const int f = header.field_of[c];
      if (f >= 0 && size_t(f) < fields.size() && !fields[f].empty()) return fields[f];
      return f >= 0 ? header.default_of[c] : std::string();
    };
    for (int c : {kName, kType, kRa, kDec, kI})
      if (size_t(header.field_of[c]) >= fields.size())
        p.Fail("too few fields: " + std::to_string(fields.size()) + ", and '" + kColumnNames[c] +
               "' is column " + std::to_string(header.field_of[c] + 1));
    Source source;
    source.name = field(kName);
    const std::string type = Lower(field(kType));
    if (type == "point")
      source.type = Type::kPoint;
    else if (type == "gaussian")
      source.type = Type::kGaussian;
    else
      p.Fail("unknown source type '" + field(kType) + "'");
    if (field(kRa).empty()) p.Fail("empty Ra");
    if (field(kDec).empty()) p.Fail("empty Dec");
    source.ra = p.Sexagesimal(field(kRa), ':', false, "Ra") * (kPi / 12.0L);
    source.dec = p.Sexagesimal(field(kDec), '.', true, "Dec") * (kPi / 180.0L);
    source.flux = p.Float(field(kI), "I");
    source.terms = p.Terms(field(kSpectralIndex));
    const std::string logarithmic = field(kLogarithmicSI);
    source.logarithmic = logarithmic.empty() ? true : p.Boolean(logarithmic);
    const std::string reference = field(kReferenceFrequency);
    if (!reference.empty()) {
      source.reference_frequency = p.Number(reference, "ReferenceFrequency");
      if (!(source.reference_frequency > 0.0)) p.Fail("ReferenceFrequency is not positive");
    } else if (!source.terms.empty()) {
      p.Fail("spectral terms without a ReferenceFrequency");
    }
    if (!field(kMajorAxis).empty()) source.major = p.Number(field(kMajorAxis), "MajorAxis");
    if (!field(kMinorAxis).empty()) source.minor = p.Number(field(kMinorAxis), "MinorAxis");
    if (!field(kOrientation).empty())
      source.orientation = p.Number(field(kOrientation), "Orientation");
    catalogue.sources_.push_back(std::move(source));
  }
  if (!have_header) {
    ++p.line;
    p.Fail("no 'Format = ...' line");
  }
  return catalogue;
}

double SourceCatalogue::ReferenceFrequency() const {
  if (header_reference_frequency_ != 0.0) return header_reference_frequency_;
  for (const Source& s : sources_)
    if (s.reference_frequency != 0.0) return s.reference_frequency;
  return 0.0;
}

std::vector<float> SourceCatalogue::FluxAt(const std::vector<double>& frequencies) const {
  const size_t n = sources_.size();
  std::vector<float> table(frequencies.size() * n);
  std::vector<float> terms;
  for (size_t i = 0; i != n; ++i) {
    const Source& s = sources_[i];
    terms.assign(1, s.flux);
    terms.insert(terms.end(), s.terms.begin(), s.terms.end());
    for (size_t g = 0; g != frequencies.size(); ++g) {
      float value = s.flux;
      if (!s.terms.empty()) {
        const double ratio = frequencies[g] / s.reference_frequency;
        if (s.logarithmic) {
          value = rdl::lp::Evaluate(terms.data(), int(terms.size()), std::log10(ratio));
        } else {  // SpectralFitter::Evaluate's loop
          const float x = float(ratio - 1.0);
          float power = 1.0f;
          for (size_t k = 1; k != terms.size(); ++k) {
            power *= x;
            value += power * terms[k];
          }
        }
      }
      table[g * n + i] = value;
    }
  }
  return table;
}

std::vector<std::pair<double, double>> SourceCatalogue::PixelPositions(
    const Geometry& g) const {
  using aocommon::ImageCoordinates;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<std::pair<double, double>> positions(sources_.size(), {nan, nan});
  size_t dropped = 0;
  for (size_t i = 0; i != sources_.size(); ++i) {
    const Source& s = sources_[i];
    long double l, m, x, y;
    ImageCoordinates::RaDecToLM<long double>(s.ra, s.dec, g.phase_centre_ra, g.phase_centre_dec,
                                             l, m);
    const long double n = ImageCoordinates::RaDecToN<long double>(
        s.ra, s.dec, g.phase_centre_ra, g.phase_centre_dec);
    if (!(l * l + m * m < 1.0L) || !(n > 0.0L)) {
      ++dropped;
      continue;
    }
    ImageCoordinates::LMToXY<long double>(l - g.l_shift, m - g.m_shift, g.pixel_scale_x,
                                          g.pixel_scale_y, g.width, g.height, x, y);
    positions[i] = {double(x), double(y)};
  }
  dropped_ = dropped;
  if (dropped != 0)
    log::Info() << "Source catalogue: " << dropped << " of " << sources_.size()
                << " sources lie off the hemisphere of the phase centre and were dropped\n";
  return positions;
}

void SourceCatalogue::CheckArguments(const Geometry& g, const std::vector<double>& frequencies,
                                     const Beam* beam) {
  const char* who = beam ? "SourceCatalogue::Restore: " : "SourceCatalogue::DrawModel: ";
  auto fail = [&](const char* why) { throw std::invalid_argument(std::string(who) + why); };
  if (g.width == 0 || g.height == 0) fail("the image is empty");
  if (g.width > (size_t(1) << 30) || g.height > (size_t(1) << 30)) fail("the image is too large");
  if (!(g.pixel_scale_x > 0.0L) || !(g.pixel_scale_y > 0.0L) || !std::isfinite(g.pixel_scale_x) ||
      !std::isfinite(g.pixel_scale_y))
    fail("a pixel scale is not positive");
  if (!std::isfinite(g.phase_centre_ra) || !std::isfinite(g.phase_centre_dec) ||
      !std::isfinite(g.l_shift) || !std::isfinite(g.m_shift))
    fail("the phase centre or a shift is not finite");
  if (frequencies.empty()) fail("no frequencies given");
  if (frequencies.size() > RDL_MAX_IMAGES) fail("more frequencies than RDL_MAX_IMAGES planes");
  for (double frequency : frequencies)
    if (!(frequency > 0.0) || !std::isfinite(frequency)) fail("a frequency is not positive");
  if (beam) {
    if (!(beam->major > 0.0L) || !(beam->minor > 0.0L) || !std::isfinite(beam->major) ||
        !std::isfinite(beam->minor))
      fail("a beam axis is not positive: a list cannot be restored without a beam");
    if (!std::isfinite(beam->pa)) fail("the beam's position angle is not finite");
  }
}

SourceCatalogue::Drawing SourceCatalogue::MakeDrawing(const Geometry& g,
                                                      const std::vector<double>& frequencies,
                                                      const Beam* beam) const {
  CheckArguments(g, frequencies, beam);
  const std::vector<std::pair<double, double>> positions = PixelPositions(g);
  const std::vector<float> flux = FluxAt(frequencies);
  const size_t n = sources_.size();
  const long double to_sigma = FwhmToSigma();
  Covariance beam_cov;
  if (beam)
    beam_cov = PixelCovariance(beam->major * to_sigma, beam->minor * to_sigma, beam->pa,
                               g.pixel_scale_x, g.pixel_scale_y);
  // the 6 sigma box never needs to be wider than the plane
  const long double cap = (long double)(std::max(g.width, g.height));

  Drawing drawing;
  std::vector<size_t> kept;
  std::vector<double> factor;
  for (size_t i = 0; i != n; ++i) {
    if (std::isnan(positions[i].first)) continue;
    const Source& s = sources_[i];
    Covariance c = beam_cov;
    const bool gaussian = s.type == Type::kGaussian && s.major > 0.0 && s.minor > 0.0;
    if (gaussian) {
      const Covariance own = PixelCovariance(
          (long double)(s.major) * kArcsec * to_sigma, (long double)(s.minor) * kArcsec * to_sigma,
          (long double)(s.orientation) * (kPi / 180.0L), g.pixel_scale_x, g.pixel_scale_y);
      c.xx += own.xx;
      c.xy += own.xy;
      c.yy += own.yy;
    }
    rdl_source_shape shape{};
    shape.x0 = positions[i].first;
    shape.y0 = positions[i].second;
    double scale = 1.0;
    if (gaussian || beam) {
      const long double det = c.Det();
      shape.qa = double(c.yy / det);
      shape.qb = double(-c.xy / det);
      shape.qc = double(c.xx / det);
      // sigma along the major axis, in pixels
      const long double mean = 0.5L * (c.xx + c.yy), diff = 0.5L * (c.xx - c.yy);
      const long double sigma = sqrtl(mean + sqrtl(diff * diff + c.xy * c.xy));
      const uint32_t half = uint32_t(std::min(ceill(6.0L * sigma), cap));
      shape.half_w = shape.half_h = half;
      // Jy/beam: the peak of the beam-convolved source; Jy/pixel: unit integral
      scale = beam ? double(sqrtl(beam_cov.Det() / det)) : double(1.0L / (2.0L * kPi * sqrtl(det)));
      if (!std::isfinite(shape.qa) || !std::isfinite(shape.qb) || !std::isfinite(shape.qc) ||
          !std::isfinite(scale))
        throw std::runtime_error("Source catalogue: source '" + s.name +
                                 "' has a degenerate shape at this pixel scale");
    }
    drawing.shapes.push_back(shape);
    kept.push_back(i);
    factor.push_back(scale);
  }
  const size_t n_kept = kept.size();
  drawing.amplitudes.resize(frequencies.size() * n_kept);
  for (size_t f = 0; f != frequencies.size(); ++f)
    for (size_t k = 0; k != n_kept; ++k)
      drawing.amplitudes[f * n_kept + k] = float(double(flux[f * n + kept[k]]) * factor[k]);
  return drawing;
}

std::vector<aocommon::Image> SourceCatalogue::DrawModel(
    gpu::Session& session, const Geometry& g, const std::vector<double>& frequencies) const {
  const Drawing drawing = MakeDrawing(g, frequencies, nullptr);
  if (drawing.shapes.size() > std::numeric_limits<uint32_t>::max())
    throw std::runtime_error("SourceCatalogue::DrawModel: more than 2^32 sources");
  const size_t plane = g.width * g.height, n_out = frequencies.size();
  session.Bind();
  gpu::Buffer out(session, n_out * plane * sizeof(float));
  gpu::Check(rdl_memset_zero(session.Handle(), out.Ptr(), n_out * plane * sizeof(float)),
             "rdl_memset_zero");
  gpu::Check(rdl_draw_sources(session.Handle(), uint32_t(drawing.shapes.size()),
                              drawing.shapes.data(), drawing.amplitudes.data(), uint32_t(n_out),
                              uint32_t(g.width), uint32_t(g.height), out.F(), plane),
             "rdl_draw_sources");
  session.Sync();
  std::vector<aocommon::Image> result;
  for (size_t f = 0; f != n_out; ++f) {
    result.emplace_back(g.width, g.height);
    session.D2H(result.back().Data(), out.F() + f * plane, plane * sizeof(float));
  }
  return result;
}

void SourceCatalogue::Restore(gpu::Session& session, float* d_images, const Geometry& g,
                              const std::vector<double>& frequencies, const Beam& beam) const {
  const Drawing drawing = MakeDrawing(g, frequencies, &beam);
  if (!d_images) throw std::invalid_argument("SourceCatalogue::Restore: no images given");
  if (drawing.shapes.size() > std::numeric_limits<uint32_t>::max())
    throw std::runtime_error("SourceCatalogue::Restore: more than 2^32 sources");
  session.Bind();
  gpu::Check(rdl_draw_sources(session.Handle(), uint32_t(drawing.shapes.size()),
                              drawing.shapes.data(), drawing.amplitudes.data(),
                              uint32_t(frequencies.size()), uint32_t(g.width), uint32_t(g.height),
                              d_images, g.width * g.height),
             "rdl_draw_sources");
}

}  // namespace radler
