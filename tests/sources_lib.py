"""Source catalogues (include/rdl_hip.h, "source catalogues";
csrc/host/source_catalogue.h): the ctypes binding of rdl_draw_sources and the
numpy float64 references of the contract, the coordinates, the two flux laws
and the Gaussian covariances. Not a test file."""
import ctypes as C
import math

import numpy as np

from rdl_lib import Rdl, RdlError, Session  # noqa: F401  (the loader, for the tests)

FWHM_TO_SIGMA = 1.0 / (2.0 * math.sqrt(2.0 * math.log(2.0)))
ARCSEC = math.pi / (180.0 * 3600.0)
LN10 = 2.302585092994045684


class SourceShape(C.Structure):
    """rdl_source_shape."""
    _fields_ = [("x0", C.c_double), ("y0", C.c_double), ("qa", C.c_double), ("qb", C.c_double),
                ("qc", C.c_double), ("half_w", C.c_uint32), ("half_h", C.c_uint32)]


assert C.sizeof(SourceShape) == 48


def shape_array(shapes):
    """shapes: rows of (x0, y0, qa, qb, qc, half_w, half_h)."""
    arr = (SourceShape * max(len(shapes), 1))()
    for i, (x0, y0, qa, qb, qc, hw, hh) in enumerate(shapes):
        arr[i] = SourceShape(float(x0), float(y0), float(qa), float(qb), float(qc), int(hw),
                             int(hh))
    return arr


def draw_sources(sess, shapes, amplitudes, dplanes, n_planes, width, height, stride=None,
                 n_sources=None):
    """rdl_draw_sources: shapes as shape_array takes them (or None), amplitudes
    (n_planes, n) float32 (or None), dplanes a DeviceArray or a c_void_p."""
    n = len(shapes) if n_sources is None else n_sources
    h_shapes = None if shapes is None else shape_array(shapes)
    if amplitudes is None:
        h_amp = None
    else:
        amplitudes = np.ascontiguousarray(amplitudes, np.float32)
        h_amp = amplitudes.ctypes.data_as(C.c_void_p)
    sess.rdl.rdl_draw_sources(sess.h, C.c_uint32(n), h_shapes, h_amp, C.c_uint32(n_planes),
                              C.c_uint32(width), C.c_uint32(height),
                              getattr(dplanes, "vp", dplanes),
                              C.c_size_t(width * height if stride is None else stride))


# ---------------------------------------------------------------- references
def round_half_up(v):
    return math.floor(v + 0.5)


def contract_sum(shapes, amplitudes, width, height):
    """The contract's sum, pixel by pixel in source order, float64:
    (sum, sum of |a g|), each (n_planes, height, width)."""
    amplitudes = np.asarray(amplitudes, np.float32).astype(np.float64)
    n_planes = amplitudes.shape[0]
    total = np.zeros((n_planes, height, width), np.float64)
    absolute = np.zeros_like(total)
    for i, (x0, y0, qa, qb, qc, hw, hh) in enumerate(shapes):
        cx, cy = round_half_up(x0), round_half_up(y0)
        xlo, xhi = max(cx - hw, 0), min(cx + hw, width - 1)
        ylo, yhi = max(cy - hh, 0), min(cy + hh, height - 1)
        if xlo > xhi or ylo > yhi:
            continue
        ys, xs = slice(int(ylo), int(yhi) + 1), slice(int(xlo), int(xhi) + 1)
        yy, xx = np.mgrid[ys, xs].astype(np.float64)
        dx, dy = xx - x0, yy - y0
        g = np.exp(-0.5 * (qa * dx * dx + 2.0 * qb * dx * dy + qc * dy * dy))
        for p in range(n_planes):
            total[p, ys, xs] += amplitudes[p, i] * g
            absolute[p, ys, xs] += abs(amplitudes[p, i]) * g
    return total, absolute


def contract_result(dest, total):
    """dest += float(sum), in float32."""
    return (np.asarray(dest, np.float32) + total.astype(np.float32)).astype(np.float32)


def contract_bound(dest, total, absolute):
    """2^-24 (|sum| + |dest + sum|) + 1e-13 sum |a g|: the two float roundings
    the contract allows, and the device's double exp against numpy's."""
    d = np.asarray(dest, np.float64)
    return 2.0 ** -24 * (np.abs(total) + np.abs(d + total)) + 1e-13 * absolute


def radec_to_lm(ra, dec, ra0, dec0):
    da = ra - ra0
    return (math.cos(dec) * math.sin(da),
            math.sin(dec) * math.cos(dec0) - math.cos(dec) * math.sin(dec0) * math.cos(da))


def lm_to_radec(l, m, ra0, dec0):
    n = math.sqrt(1.0 - l * l - m * m)
    return (ra0 + math.atan2(l, n * math.cos(dec0) - m * math.sin(dec0)),
            math.asin(m * math.cos(dec0) + n * math.sin(dec0)))


def radec_to_xy(ra, dec, width, height, scale_x, scale_y, ra0, dec0, l_shift=0.0, m_shift=0.0):
    l, m = radec_to_lm(ra, dec, ra0, dec0)
    return width / 2 - (l - l_shift) / scale_x, height / 2 + (m - m_shift) / scale_y


def xy_to_radec(x, y, width, height, scale_x, scale_y, ra0, dec0, l_shift=0.0, m_shift=0.0):
    l = (width / 2 - x) * scale_x + l_shift
    m = (y - height / 2) * scale_y + m_shift
    return lm_to_radec(l, m, ra0, dec0)


def format_ra(ra):
    """HH:MM:SS.sss, sign kept."""
    return _sexagesimal(ra * 12.0 / math.pi, ":")


def format_dec(dec):
    return _sexagesimal(dec * 180.0 / math.pi, ".")


def _sexagesimal(units, delimiter):
    parts = int(round(abs(units) * 3600000.0))
    text = "%02d%s%02d%s%02d.%03d" % (parts // 3600000, delimiter, parts // 60000 % 60, delimiter,
                                     parts // 1000 % 60, parts % 1000)
    return ("-" if units < 0 and parts else "") + text


def log_flux(terms, frequency, reference):
    """S = t0 10^(t1 lg + t2 lg^2 + ...), float64."""
    lg = math.log10(frequency / reference)
    e = 0.0
    for t in reversed([float(np.float32(t)) for t in terms[1:]]):
        e = (e + t) * lg
    return float(np.float32(terms[0])) * math.exp(LN10 * e)


def polynomial_flux(terms, frequency, reference):
    """SpectralFitter::Evaluate's float loop in x = nu / nu_ref - 1: float32."""
    x = np.float32(frequency / reference - 1.0)
    value, power = np.float32(terms[0]), np.float32(1.0)
    for t in terms[1:]:
        power = np.float32(power * x)
        value = np.float32(value + np.float32(power * np.float32(t)))
    return value


def pixel_covariance(major, minor, pa, scale_x, scale_y):
    """FWHM axes and position angle in radians (restore.h's beam_pa: the major
    axis along (cos, sin)(pa + pi/2) in (l, m)) -> the 2 x 2 covariance in
    pixels, through J = diag(-1/scale_x, 1/scale_y)."""
    a = pa + 0.5 * math.pi
    u = np.array([math.cos(a), math.sin(a)])
    v = np.array([-math.sin(a), math.cos(a)])
    cov = (major * FWHM_TO_SIGMA) ** 2 * np.outer(u, u) + \
        (minor * FWHM_TO_SIGMA) ** 2 * np.outer(v, v)
    j = np.diag([-1.0 / scale_x, 1.0 / scale_y])
    return j @ cov @ j.T


def gaussian_of(cov, x0, y0, width, height):
    """exp(-1/2 d^T cov^-1 d) on every pixel of the plane, float64."""
    q = np.linalg.inv(cov)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    dx, dy = xx - x0, yy - y0
    return np.exp(-0.5 * (q[0, 0] * dx * dx + 2.0 * q[0, 1] * dx * dy + q[1, 1] * dy * dy))


def shape_of(cov, x0, y0, width, height):
    """The rdl_source_shape of a covariance: its inverse and the 6 sigma box."""
    q = np.linalg.inv(cov)
    sigma = math.sqrt(float(np.linalg.eigvalsh(cov)[-1]))
    half = int(min(math.ceil(6.0 * sigma), max(width, height)))
    return (x0, y0, q[0, 0], q[0, 1], q[1, 1], half, half)
