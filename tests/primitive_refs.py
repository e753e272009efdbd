"""Plain references of the streaming primitives of include/rdl_hip.h.

One function per entry point, written from the header's contract and the
reference lines it cites, in NumPy at float64 or wider: never from the kernel.
tests/test_primitive_refs.py checks these against the oracle and hand-worked
cases before tests/test_primitives_gpu.py lets them judge a kernel.

Two tolerances are derived here rather than measured:

* order-free double reductions: any order of summing n doubles errs by at most
  n * 2^-53 * sum|term_i| to first order, so a device sum must lie within
  n * 2^-52 * sum|term_i| of math.fsum of the same float64 terms
  (reduction_tolerance);
* "within 1 float32 ulp": a float64 value computed two ways that differ by a
  few double ulp rounds to float32 values at most one step apart (ulp_distance).
"""
import math
from fractions import Fraction

import numpy as np

FLT_LOWEST = -np.finfo(np.float32).max

BOX_COPY, BOX_COPY_MASKED, BOX_COPY_ZERO, BOX_ADD = 0, 1, 2, 3  # rdl_hip.h


# ------------------------------------------------------------ shared helpers
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fma_f32(a, alpha, d):
    """float32 of an exactly rounded double fma(a, alpha, d), elementwise over
    (a few thousand) sampled elements: the sum is formed exactly in rationals,
    rounded once to double and once to float."""
    alpha = Fraction(float(alpha))
    return np.array([np.float32(float(Fraction(float(x)) * alpha + Fraction(float(y))))
                     for x, y in zip(np.ravel(a), np.ravel(d))], np.float32)


def ordered(a):
    """float32 -> int64 that steps by one per representable value (+-0 equal)."""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def ulp_distance(a, b):
    """Representable float32 values between a and b (both finite)."""
    return np.abs(ordered(a) - ordered(b))


def reduction_tolerance(terms):
    """The bound on |any-order double sum - exact sum| of these float64 terms."""
    t = np.asarray(terms, np.float64).ravel()
    return t.size * 2.0 ** -52 * math.fsum(np.abs(t))


def exact_sum(terms):
    return math.fsum(np.asarray(terms, np.float64).ravel())


def exact_fma_inputs(n, seed=0):
    """(a, alpha, dest) for which float64 a * alpha + dest is exact, so that
    np.float32 of it is the once-rounded fused multiply-add: a = k 2^-12 with
    |k| < 2^15, alpha = 45877 2^-16, |dest| in [2^-4, 8). The product is a
    multiple of 2^-28 below 8 and dest a multiple of 2^-27 below 8: the sum
    needs 32 bits."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-(2 ** 15) + 1, 2 ** 15, n)
    a = (k * 2.0 ** -12).astype(np.float32)
    alpha = np.float32(45877 * 2.0 ** -16)
    dest = rng.uniform(2.0 ** -4, 8.0, n).astype(np.float32)
    dest *= np.where(rng.integers(0, 2, n) == 0, np.float32(1), np.float32(-1))
    return a, alpha, dest


# ------------------------------------------------- elementwise (image_set.cc)
def axpy_assign(a, alpha):
    """rdl_axpy, assign = 1: dest = a * alpha, one float multiply."""
    return np.asarray(a, np.float32) * np.float32(alpha)


def axpy_fused_exact(dest, a, alpha):
    """rdl_axpy, assign = 0, for exact_fma_inputs: float(a * alpha + dest) with
    the inner value exact in float64."""
    return (np.asarray(a, np.float64) * np.float64(np.float32(alpha))
            + np.asarray(dest, np.float64)).astype(np.float32)


def scale(dest, alpha):
    return np.asarray(dest, np.float32) * np.float32(alpha)


def add(dest, a):
    return np.asarray(dest, np.float32) + np.asarray(a, np.float32)


def axpy_f64_scale(dest, alpha):
    """rdl_axpy_f64 mode 1: float(double(dest) * alpha)."""
    return (np.asarray(dest, np.float64) * np.float64(alpha)).astype(np.float32)


def axpy_f64_unfused(dest, a, alpha):
    """rdl_axpy_f64 mode 0 with the product rounded to double before the add:
    one float64 rounding away from the fused form, so at most 1 float32 ulp."""
    return (np.asarray(a, np.float64) * np.float64(alpha)
            + np.asarray(dest, np.float64)).astype(np.float32)


def convert(src, to_f64):
    return np.asarray(src, np.float32).astype(np.float64) if to_f64 else \
        np.asarray(src, np.float64).astype(np.float32)


def integrate_linear(images, weights):
    """GetLinearIntegrated with one polarization in float64:
    sum_c w_c image_c / sum_c w_c over the channels of non-zero weight."""
    w = np.asarray(weights, np.float64)
    img = np.asarray(images, np.float64)
    return np.tensordot(w, img, 1) / w.sum()


def box(dst, dst_x, dst_y, src, src_x, src_y, w, h, mask, op):
    """rdl_box on 2-D arrays (their widths are the strides); mask is box-local
    (h x w) or None. Returns the new dst."""
    out = np.array(dst, np.float32)
    s = np.asarray(src, np.float32)[src_y:src_y + h, src_x:src_x + w]
    d = out[dst_y:dst_y + h, dst_x:dst_x + w]
    m = np.ones((h, w), bool) if mask is None else np.asarray(mask).reshape(h, w) != 0
    if op == BOX_COPY:
        d[...] = s
    elif op == BOX_COPY_MASKED:
        d[m] = s[m]
    elif op == BOX_COPY_ZERO:
        d[...] = np.where(m, s, np.float32(0))
    elif op == BOX_ADD:
        d[...] = d + s
    else:
        raise ValueError(op)
    return out


def bits_differ(a, b):
    """Any differing 32-bit word (+0.0 and -0.0 differ, equal NaN patterns do not)."""
    return bool(np.any(np.ascontiguousarray(a).view(np.uint32)
                       != np.ascontiguousarray(b).view(np.uint32)))


# ----------------------------------------------------------- Trim / Untrim
def untrim(src, pw, ph):
    """Image::Untrim: the h x w image in a zeroed ph x pw plane at offset
    ((pw - w) / 2, (ph - h) / 2), rounded down."""
    s = np.asarray(src, np.float32)
    h, w = s.shape
    ox, oy = (pw - w) // 2, (ph - h) // 2
    out = np.zeros((ph, pw), np.float32)
    out[oy:oy + h, ox:ox + w] = s
    return out


def trim(src, w, h):
    """Image::Trim: the window Untrim fills."""
    s = np.asarray(src, np.float32)
    ph, pw = s.shape
    ox, oy = (pw - w) // 2, (ph - h) // 2
    return s[oy:oy + h, ox:ox + w].copy()


def periodic_extend(src, pw, ph, sx, sy):
    """dest[y][x] = src[(y - sy) mod h][(x - sx) mod w]."""
    s = np.asarray(src, np.float32)
    h, w = s.shape
    yy = (np.arange(ph) - sy) % h
    xx = (np.arange(pw) - sx) % w
    return s[np.ix_(yy, xx)]


# --------------------------------------------------- local RMS (rms_image.cc)
def square(src):
    s = np.asarray(src, np.float32)
    return s * s


def multiply(a, b):
    return np.asarray(a, np.float32) * np.asarray(b, np.float32)


def rms_finish(d, norm):
    """rms_image.cc:33: val = sqrt(val * norm) in double."""
    return np.sqrt(np.asarray(d, np.float64) * np.float64(norm)).astype(np.float32)


def rms_negativity_limit(rms, mn):
    """rms_image.cc:89-92: max<float>(rms, |min| * (1.5 / 5.0)); std::max
    keeps its first argument on equality."""
    r = np.asarray(rms, np.float32)
    lim = (np.abs(np.asarray(mn, np.float32)).astype(np.float64) * (1.5 / 5.0)).astype(np.float32)
    return np.where(r < lim, lim, r)


def rms_factor(rms, strength):
    """MakeRmsFactorImage (rms_image.cc:95-125) -> (factor image as float64
    before the final float rounding, lowest rms). ValueError where the
    reference throws."""
    r = np.asarray(rms, np.float32)
    stddev = np.float64(r.min())
    if stddev < 0.0:
        raise ValueError("RMS image can only contain values >= 0")
    v = r.astype(np.float64)
    if strength == 0.0:
        return np.ones_like(v), stddev
    nz = v != 0.0
    out = np.zeros_like(v)
    q = stddev / v[nz]
    out[nz] = q if strength == 1.0 else np.power(q, strength)
    return out, stddev


def place_gaussian(w, h, boxsize, pl, pm, sigma_major, sigma_minor, angle):
    """schaapcommon RestoreImage's kernel as rdl_place_gaussian states it: a
    box x box Gaussian of peak 1, centre (box/2, box/2) wrapped to the origin
    of a zeroed plane. float64; also returns the mask of written pixels."""
    out = np.zeros((h, w), np.float64)
    written = np.zeros((h, w), bool)
    c = boxsize // 2
    y, x = np.mgrid[0:boxsize, 0:boxsize]
    l = (c - x).astype(np.float64) * pl
    m = (y - c).astype(np.float64) * pm
    ca, sa = math.cos(angle), math.sin(angle)
    lt = (l * ca + m * sa) / sigma_major
    mt = (-l * sa + m * ca) / sigma_minor
    g = np.exp(-0.5 * (lt * lt + mt * mt))
    py, px = (y - c) % h, (x - c) % w
    out[py, px] = g
    written[py, px] = True
    return out, written


def _sliding_min_lines(a, window):
    """Along the last axis: min over [max(k, half) - half, min(k, len - half) + half)."""
    half = window // 2
    n = a.shape[-1]
    out = np.empty_like(a)
    for k in range(n):
        out[..., k] = a[..., max(k, half) - half:min(k, n - half) + half].min(axis=-1)
    return out


def sliding_min(image, window):
    """rms_image::SlidingMinimum (rms_image.cc:36-70): rows, then columns."""
    a = np.asarray(image, np.float32)
    rows = _sliding_min_lines(a, window)
    return np.ascontiguousarray(_sliding_min_lines(rows.T, window).T)


# ------------------------------------------- component optimisation pieces
def masked_copy(model, src, sign):
    """dst = model != 0 ? sign * src : 0 (NaN != 0, so it copies)."""
    m = np.asarray(model, np.float32)
    return np.where(m != 0, np.float32(sign) * np.asarray(src, np.float32), np.float32(0))


def masked_add(model, values):
    m = np.asarray(model, np.float32)
    return np.where(m != 0, m + np.asarray(values, np.float32), m)


# -------------------------------------------------------- order statistics
def select_kth(v, use_center, center, k):
    """k-th smallest of v (of |v - center| in float when use_center)."""
    x = np.asarray(v, np.float32)
    if use_center:
        x = np.abs(x - np.float32(center))
    return np.sort(x)[k]


def median(v, use_center, center):
    x = np.asarray(v, np.float32)
    if use_center:
        x = np.abs(x - np.float32(center))
    s = np.sort(x)
    n = s.size
    return s[n // 2] if n % 2 else np.float32(0.5) * (s[n // 2 - 1] + s[n // 2])


# ---------------------------------- IUWT pieces (iuwt_deconvolution_algorithm.cc)
def max_abs_loops(data, xb, yb, allow_negative, mask=None):
    """GetMaxAbsWithMask / WithoutMask (:112-167) as written, pixel by pixel.
    -> (found, x, y, value)."""
    d = np.asarray(data, np.float32)
    h, w = d.shape
    x, y, best = w, h, np.float32(FLT_LOWEST)
    for yi in range(yb, h - yb):
        for xi in range(xb, w - xb):
            if mask is not None and not mask[yi, xi]:
                continue
            val = np.abs(d[yi, xi]) if allow_negative else d[yi, xi]
            if val > best:
                best, x, y = val, xi, yi
    return int(x < w), x, y, best


def max_abs(data, xb, yb, allow_negative, mask=None):
    """The same loop in whole-array form: the strict '>' from lowest() keeps
    the first row-major position of the largest qualifying value."""
    d = np.asarray(data, np.float32)
    h, w = d.shape
    val = np.abs(d) if allow_negative else d
    ok = np.zeros((h, w), bool)
    ok[yb:h - yb, xb:w - xb] = True
    if mask is not None:
        ok &= np.asarray(mask).reshape(h, w) != 0
    with np.errstate(invalid="ignore"):
        ok &= val > np.float32(FLT_LOWEST)   # NaN, -inf and lowest() never pass
    if not ok.any():
        return 0, w, h, np.float32(FLT_LOWEST)
    i = int(np.argmax(np.where(ok, val, -np.inf)))   # first index of the maximum
    return 1, i % w, i // w, val.ravel()[i]


def exceeds_threshold(v, t):
    """image_analysis.cc:9-15."""
    v = np.asarray(v, np.float32)
    t = np.float32(t)
    with np.errstate(invalid="ignore"):
        return v > t if t >= 0 else (v < t) | (v > -t)


def iuwt_select(coeffs, min_scale, end_scale, thresholds, xb, yb, prior=None):
    """SelectStructures' resulting mask (end_scale planes) and its count."""
    c = np.asarray(coeffs, np.float32)
    _, h, w = c.shape
    inside = np.zeros((h, w), bool)
    inside[yb:h - yb, xb:w - xb] = True
    if prior is not None:
        inside &= np.asarray(prior).reshape(h, w) != 0
    mask = np.zeros((end_scale, h, w), np.uint8)
    for s in range(min_scale, end_scale):
        mask[s] = inside & exceeds_threshold(c[s], thresholds[s])
    return mask, int(mask.sum())


def iuwt_apply_mask(coeffs, mask):
    c = np.asarray(coeffs, np.float32)
    return np.where(np.asarray(mask).reshape(c.shape) != 0, c, np.float32(0))


def bbox_rows(image):
    """BoundingBox's test per row (:183-213): m = max(max, -min); first and
    last x with double(|v|) > double(m) * 0.01, -1 where a row has none."""
    a = np.asarray(image, np.float32)
    h, w = a.shape
    first = np.full(h, -1, np.int32)
    last = np.full(h, -1, np.int32)
    if a.size == 0:
        return first, last
    m = max(a.max(), -a.min())
    hit = np.abs(a).astype(np.float64) > np.float64(m) * 0.01
    any_ = hit.any(axis=1)
    first[any_] = hit.argmax(axis=1)[any_]
    last[any_] = (w - 1 - hit[:, ::-1].argmax(axis=1))[any_]
    return first, last


def dot_terms(a, b):
    return np.asarray(a, np.float64) * np.asarray(b, np.float64)


def snr_terms(noisy, model):
    """-> (model terms m^2, noise terms double(float(m - n))^2): m - n is a
    float32 subtraction here, widened afterwards."""
    n, m = np.asarray(noisy, np.float32), np.asarray(model, np.float32)
    return m.astype(np.float64) ** 2, (m - n).astype(np.float64) ** 2


def rms(v):
    """float(sqrt(sum v^2 / n)) from the exact sum."""
    x = np.asarray(v, np.float64).ravel()
    return np.float32(math.sqrt(exact_sum(x * x) / x.size))


# ------------------------------------------------------------------ spectra
def spectrum_multiply(a, b, scale):
    """-> (float64 complex product * scale, bound on the real parts' error,
    bound on the imaginary parts'): float products and their sum or difference,
    fused or not, err by at most 4 * 2^-24 * (|p| + |q|) before the scale, and
    the scale multiplies that and adds one more rounding of the result."""
    a = np.asarray(a, np.complex64).astype(np.complex128)
    b = np.asarray(b, np.complex64).astype(np.complex128)
    s = abs(float(np.float32(scale)))
    ref = a * b * float(np.float32(scale))
    u = 4 * 2.0 ** -24
    tol_re = u * (np.abs(a.real * b.real) + np.abs(a.imag * b.imag)) * s
    tol_im = u * (np.abs(a.real * b.imag) + np.abs(a.imag * b.real)) * s
    return ref, tol_re, tol_im


def fft_inverse(spectrum, w, h):
    """Unnormalised real inverse of an h x (w/2+1) spectrum."""
    return np.fft.irfft2(np.asarray(spectrum, np.complex128), s=(h, w)) * (w * h)


# ------------------------------------------- what is done with the model
def unpack_positions(pos):
    p = np.asarray(pos, np.uint32)
    return (p & 0xffff).astype(np.int64), (p >> 16).astype(np.int64)


def model_plane(pos, values, dest_w, dest_h, ox, oy, dtype):
    """GetFullIndividualModel into a zeroed plane at offset (ox, oy); the
    float -> double widening is exact."""
    x, y = unpack_positions(pos)
    out = np.zeros((dest_h, dest_w), dtype)
    out[y + oy, x + ox] = np.asarray(values, np.float32).astype(dtype)
    return out


def model_rows(pos, values, n_rows, oy):
    """rows[y + oy] = 1 where row y holds a non-zero model value."""
    _, y = unpack_positions(pos)
    out = np.zeros(n_rows, np.uint8)
    out[y[np.asarray(values, np.float32) != 0] + oy] = 1
    return out


def model_masked(dest, pos, values, rows, oy):
    """rdl_subminor_model_masked on an existing plane: marked rows zeroed, then
    every selected pixel stored (zero values included)."""
    out = np.array(dest, np.float32)
    marked = np.asarray(rows)[oy:oy + out.shape[0]] != 0
    out[marked] = 0
    x, y = unpack_positions(pos)
    out[y, x] = np.asarray(values, np.float32)
    return out


def update_mask(mask, pos, values_per_image):
    """UpdateAutoMask (subminor_loop.cc:220-228): set where any image's model
    value is non-zero, untouched elsewhere."""
    out = np.array(mask, np.uint8)
    x, y = unpack_positions(pos)
    any_ = (np.asarray(values_per_image, np.float32) != 0).any(axis=0)
    out[y[any_], x[any_]] = 1
    return out
