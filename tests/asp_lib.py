"""The adaptive-scale-pixel primitives (include/rdl_hip.h, "adaptive scale
pixel"): ctypes bindings of the three entry points and their numpy float64
references, including the Levenberg-Marquardt driver with the product's rules
(csrc/host/gaussian_fit.h). Not a test file.

Conventions, as in the header: x is the column and y the row index, FWHMs are
in pixels, the position angle runs from +x towards +y, and
params = (A, x0, y0, FWHM_maj, FWHM_min, pa).
"""
import ctypes as C

import numpy as np

from rdl_lib import Rdl, RdlError, Session  # noqa: F401  (the loader, for the tests)

FWHM_TO_SIGMA = 1.0 / (2.0 * np.sqrt(2.0 * np.log(2.0)))
N_SUMS = 28

# csrc/host/gaussian_fit.h
LM_LAMBDA_START = 1e-3
LM_LAMBDA_MIN = 1e-12
LM_LAMBDA_MAX = 1e12
LM_STEP_TOLERANCE = 1e-10
LM_DECREASE_TOLERANCE = 1e-14
LM_MAX_EVALUATIONS = 100
FIT_MAX_ROUNDS = 5


# ------------------------------------------------------------------ bindings
def fit_sums(sess, dimg, width, height, box, params):
    """rdl_gaussian_fit_sums: the 28 doubles for box = (x, y, w, h)."""
    p = (C.c_double * 6)(*[float(v) for v in params])
    out = (C.c_double * N_SUMS)()
    sess.rdl.rdl_gaussian_fit_sums(sess.h, dimg.vp, C.c_uint32(width), C.c_uint32(height),
                                   C.c_uint32(box[0]), C.c_uint32(box[1]), C.c_uint32(box[2]),
                                   C.c_uint32(box[3]), p, out)
    return np.array(out, np.float64)


def draw_gaussian(sess, dplane, width, height, x0, y0, fmaj, fmin, pa, flux):
    """dplane: a DeviceArray, or the c_void_p of a plane inside one."""
    sess.rdl.rdl_draw_gaussian(sess.h, getattr(dplane, "vp", dplane), C.c_uint32(width),
                               C.c_uint32(height), C.c_double(x0), C.c_double(y0),
                               C.c_double(fmaj), C.c_double(fmin), C.c_double(pa),
                               C.c_double(flux))


def weighted_values(sess, dplanes, n_planes, width, height, centres, fmaj, fmin, pa,
                    stride=None):
    cx = (C.c_uint32 * n_planes)(*[int(c[0]) for c in centres])
    cy = (C.c_uint32 * n_planes)(*[int(c[1]) for c in centres])
    out = (C.c_double * n_planes)()
    sess.rdl.rdl_gaussian_weighted_values(
        sess.h, dplanes.vp, C.c_size_t(width * height if stride is None else stride),
        C.c_uint32(n_planes), C.c_uint32(width), C.c_uint32(height), cx, cy, C.c_double(fmaj),
        C.c_double(fmin), C.c_double(pa), out)
    return np.array(out, np.float64)


# ---------------------------------------------------------------- references
def gaussian_uv(x, y, x0, y0, pa):
    dx, dy = x - x0, y - y0
    cs, sn = np.cos(pa), np.sin(pa)
    return dx * cs + dy * sn, dy * cs - dx * sn


def gaussian(x, y, x0, y0, fmaj, fmin, pa):
    """g(x, y) of the header, float64."""
    u, v = gaussian_uv(np.asarray(x, np.float64), np.asarray(y, np.float64), x0, y0, pa)
    smaj, smin = fmaj * FWHM_TO_SIGMA, fmin * FWHM_TO_SIGMA
    return np.exp(-0.5 * (u * u / (smaj * smaj) + v * v / (smin * smin)))


def unit_norm(fmaj, fmin):
    return 1.0 / (2.0 * np.pi * fmaj * FWHM_TO_SIGMA * fmin * FWHM_TO_SIGMA)


def fit_sums_ref(image, box, params):
    """The 28 sums over box = (x, y, w, h) of a 2-D image, float64."""
    a, x0, y0, fmaj, fmin, pa = [float(v) for v in params]
    bx, by, bw, bh = box
    yy, xx = np.mgrid[by:by + bh, bx:bx + bw].astype(np.float64)
    u, v = gaussian_uv(xx, yy, x0, y0, pa)
    cs, sn = np.cos(pa), np.sin(pa)
    smaj, smin = fmaj * FWHM_TO_SIGMA, fmin * FWHM_TO_SIGMA
    um, vm = u / (smaj * smaj), v / (smin * smin)
    e = np.exp(-0.5 * (u * um + v * vm))
    ae = a * e
    r = np.asarray(image, np.float64)[by:by + bh, bx:bx + bw] - ae
    j = [e,
         ae * (um * cs - vm * sn),
         ae * (um * sn + vm * cs),
         ae * (u * um / fmaj),
         ae * (v * vm / fmin),
         ae * (u * v * (1.0 / (smin * smin) - 1.0 / (smaj * smaj)))]
    out = []
    for i in range(6):
        for k in range(i, 6):
            out.append(np.sum(j[i] * j[k]))
    for i in range(6):
        out.append(np.sum(j[i] * r))
    out.append(np.sum(r * r))
    return np.array(out, np.float64)


def half_side(fmaj, width, height):
    return int(min(np.ceil(6.0 * fmaj * FWHM_TO_SIGMA), max(width, height)))


def draw_ref(plane, x0, y0, fmaj, fmin, pa, flux):
    """rdl_draw_gaussian on a float32 plane: evaluated in float64, rounded once,
    added in float32, inside the clipped 6 sigma box only."""
    out = np.array(plane, np.float32, copy=True)
    h, w = out.shape
    half = half_side(fmaj, w, h)
    x_lo, x_hi = max(0.0, np.floor(x0 - half)), min(w - 1.0, np.ceil(x0 + half))
    y_lo, y_hi = max(0.0, np.floor(y0 - half)), min(h - 1.0, np.ceil(y0 + half))
    if x_lo > x_hi or y_lo > y_hi:
        return out
    ys, xs = slice(int(y_lo), int(y_hi) + 1), slice(int(x_lo), int(x_hi) + 1)
    yy, xx = np.mgrid[ys, xs].astype(np.float64)
    value = (flux * unit_norm(fmaj, fmin)) * gaussian(xx, yy, x0, y0, fmaj, fmin, pa)
    out[ys, xs] = out[ys, xs] + value.astype(np.float32)
    return out


def weighted_value_ref(plane, cx, cy, fmaj, fmin, pa):
    """sum of w(dx, dy) plane[cy + dy][cx + dx] over the 6 sigma box, float64."""
    h, w = plane.shape
    half = half_side(fmaj, w, h)
    ys = slice(max(0, cy - half), min(h - 1, cy + half) + 1)
    xs = slice(max(0, cx - half), min(w - 1, cx + half) + 1)
    yy, xx = np.mgrid[ys, xs].astype(np.float64)
    wgt = unit_norm(fmaj, fmin) * gaussian(xx, yy, float(cx), float(cy), fmaj, fmin, pa)
    return float(np.sum(wgt * np.asarray(plane, np.float64)[ys, xs]))


# ------------------------------------------------- the fit driver, restated
def _tri(i, k):
    return i * 6 - i * (i - 1) // 2 + (k - i)


def normalise(p):
    if p[4] > p[3]:
        p[3], p[4] = p[4], p[3]
        p[5] += np.pi / 2
    p[5] -= np.pi * np.floor(p[5] / np.pi + 0.5)
    return p


def levenberg_marquardt(sums, p, free):
    """sums(p) -> the 28 values; p (6 floats) is fitted in place."""
    p = [float(v) for v in p]
    cur = sums(p)
    evaluations = 1
    lam = LM_LAMBDA_START
    while evaluations < LM_MAX_EVALUATIONS:
        idx = [i for i in range(6) if free[i] and cur[_tri(i, i)] > 0.0]
        if not idx:
            break
        n = len(idx)
        a = np.empty((n, n))
        for r in range(n):
            for c in range(n):
                a[r, c] = cur[_tri(min(idx[r], idx[c]), max(idx[r], idx[c]))]
        a[np.diag_indices(n)] *= 1.0 + lam
        b = np.array([cur[21 + i] for i in idx])
        accepted = False
        try:
            delta = np.linalg.solve(a, b)
        except np.linalg.LinAlgError:
            delta = None
        if delta is not None:
            trial = list(p)
            for r in range(n):
                trial[idx[r]] += delta[r]
            if trial[3] > 0.0 and trial[4] > 0.0 and np.all(np.isfinite(trial)):
                new = sums(trial)
                evaluations += 1
                accepted = new[27] < cur[27]
        if accepted:
            step = max(abs(delta[r]) / max(abs(trial[idx[r]]), 1.0) for r in range(n))
            done = step < LM_STEP_TOLERANCE or cur[27] - new[27] <= LM_DECREASE_TOLERANCE * cur[27]
            p, cur = trial, new
            lam = max(lam / 10.0, LM_LAMBDA_MIN)
            if done:
                break
        else:
            lam *= 10.0
            if lam > LM_LAMBDA_MAX:
                break
    return normalise(p)


def box_side(major):
    side = max(10.0, np.ceil(10.0 * major))
    if not side < 1e9:
        side = 1e9
    n = int(side)
    return n + (n & 1)


def make_box(width, height, side, x, y):
    """(box, whole) or (None, False) when the box misses the image."""
    if side >= width and side >= height:
        return (0, 0, width, height), True
    if not (np.isfinite(x) and np.isfinite(y)) or abs(x) > 1e9 or abs(y) > 1e9:
        return None, False
    half = side // 2
    # llround: halves away from zero
    x0 = int(np.floor(abs(x) + 0.5) * np.sign(x)) - half
    y0 = int(np.floor(abs(y) + 0.5) * np.sign(y)) - half
    xa, xb = min(max(x0, 0), width), min(max(x0 + side, 0), width)
    ya, yb = min(max(y0, 0), height), min(max(y0 + side, 0), height)
    if xb <= xa or yb <= ya:
        return None, False
    return (xa, ya, xb - xa, yb - ya), False


def fit_rounds_ref(image, p, free):
    h, w = image.shape
    p = [float(v) for v in p]
    side = box_side(p[3])
    for _ in range(FIT_MAX_ROUNDS):
        box, whole = make_box(w, h, side, p[1], p[2])
        if box is None:
            break
        p = levenberg_marquardt(lambda q, box=box: fit_sums_ref(image, box, q), p, free)
        if whole:
            break
        new_side = box_side(p[3])
        if new_side == side:
            break
        side = new_side
    return p


def fit_full_ref(image, amplitude, x, y, major, minor, pa):
    """Fit2DGaussianFull on a 2-D image: (A, x, y, major, minor, pa)."""
    return tuple(fit_rounds_ref(image, [amplitude, x, y, major, minor, pa], [True] * 6))


def fit_centred_ref(image, beam_estimate):
    """Fit2DGaussianCentred: (major, minor, pa)."""
    h, w = image.shape
    p = [float(image[h // 2, w // 2]), w // 2, h // 2, beam_estimate, beam_estimate, 0.0]
    return tuple(fit_rounds_ref(image, p, [False, False, False, True, True, True])[3:])


def deconvolve_ref(major, minor, pa, psf_major, psf_minor, psf_pa):
    """The 2 x 2 second-moment subtraction: (major, minor, pa), NaNs when the
    difference is not positive definite."""
    def moments(a, b, t):
        r = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
        return r @ np.diag([a * a, b * b]) @ r.T
    d = moments(major, minor, pa) - moments(psf_major, psf_minor, psf_pa)
    vals, vecs = np.linalg.eigh(d)
    if not vals[0] > 0.0:
        return (np.nan, np.nan, np.nan)
    t = np.arctan2(vecs[1, 1], vecs[0, 1])
    t -= np.pi * np.floor(t / np.pi + 0.5)
    return (float(np.sqrt(vals[1])), float(np.sqrt(vals[0])), float(t))
