"""rdl_component_terms: the batched spectral fit of a component list (one lane
per component) against the host SpectralFitter.fit, which ComponentList.write
calls once per component.

Tolerances:
  polynomial  |d| <= 2^-23 |term| + 1e-12 sum_c |fit_tc v_c|: one float
              rounding of a double sum;
  forced      t_1.. bit-equal to the planes, t_0 within 2 float ulps;
  log-poly    terms within rtol 2e-5, atol 2e-5 max(1, max|terms|), the bound
              between two implementations of this fit (tests/test_spectral.py),
              and the spectra evaluated from both term sets within rtol 1e-4,
              atol 1e-6 max|v|.
"""
import ctypes as C
import math

import numpy as np
import pytest

from radler_import import radler as rd
from rdl_lib import RdlError, Session, logpoly

pytestmark = pytest.mark.gpu

MODE = rd.SpectralFittingMode
POLYNOMIAL, LOGPOLY, FORCED = 0, 1, 2
W, H = 40, 24  # forced-term planes
COUNTS = [1, 63, 64, 65, 256, 257]
# one launch covers 262,144 components (rdl_component_terms' grids): this
# count goes round the grid-stride loop
BIG = 264_001
SAMPLE = 2000


class ForcedTerms(C.Structure):
    """rdl_forced_terms"""
    _fields_ = [("d_planes", C.c_void_p), ("plane_stride", C.c_size_t), ("pitch", C.c_uint32),
                ("rows", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32),
                ("weights", C.c_float * 16)]


@pytest.fixture(scope="module")
def sess():
    s = Session(0)
    yield s
    s.close()


def frequencies(n):
    return list(np.linspace(100e6, 200e6, n)) if n > 1 else [150e6]


def weights(n, zero=None):
    w = [1.0 + 0.25 * (c % 3) for c in range(n)]
    if zero is not None:
        w[zero] = 0.0
    return w


def spectra(rng, fitter, n):
    """Power laws with curvature and 1 % noise, of either sign of index."""
    f = np.asarray(fitter.frequencies)
    x = np.log10(f / fitter.reference_frequency)[None, :]
    amp = rng.uniform(0.05, 3.0, (n, 1))
    alpha = rng.uniform(-1.5, 0.5, (n, 1))
    beta = rng.uniform(-0.5, 0.5, (n, 1))
    v = amp * 10.0 ** (alpha * x + beta * x * x)
    v *= 1.0 + 0.01 * rng.standard_normal(v.shape)
    return v.astype(np.float32)


class Case:
    """A fitter, its device description and, in forced mode, its planes."""

    def __init__(self, sess, mode, n_ch, n_terms, zero=None):
        self.sess, self.mode, self.n_ch, self.n_terms = sess, mode, n_ch, n_terms
        f, w = frequencies(n_ch), weights(n_ch, zero)
        self.forced, self.planes, self.d_planes = None, None, None
        if mode == POLYNOMIAL:
            self.fitter = rd.SpectralFitter(MODE.polynomial, n_terms, f, w)
            self.map = np.ascontiguousarray(self.fitter.fit_matrix, np.float64)
            self.fitted = np.asarray([x > 0 for x in w], np.uint8)
            self.lp = None
        else:
            self.fitter = rd.SpectralFitter(
                MODE.log_polynomial if mode == LOGPOLY else MODE.forced_terms, n_terms, f, w)
            self.lp = logpoly(f, w, n_terms)
            for c in range(n_ch):  # the host fitter's own reference frequency
                self.lp.lg[c] = math.log10(f[c] / self.fitter.reference_frequency)
        if mode == FORCED:
            rng = np.random.default_rng(n_ch * 16 + n_terms)
            self.planes = rng.uniform(-1.2, 0.4, (n_terms - 1, H, W)).astype(np.float32)
            self.fitter.set_forced_terms(list(self.planes))
            self.forced = ForcedTerms()
            if n_terms > 1:
                self.d_planes = sess.array(self.planes)
                self.forced.d_planes = self.d_planes.ptr
            self.forced.plane_stride, self.forced.pitch, self.forced.rows = W * H, W, H
            for c in range(n_ch):
                self.forced.weights[c] = w[c]

    def positions(self, rng, n):
        xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)]).astype(np.uint32)
        corners = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
        for i, c in enumerate(corners[:n]):
            xy[:, i] = c
        return np.ascontiguousarray(xy)

    def device(self, values, xy=None, width=W, height=H, n_terms=None, d_values=True):
        """terms (n, n_terms) of values (n, n_ch) by rdl_component_terms"""
        n = len(values)
        n_terms = self.n_terms if n_terms is None else n_terms
        d_v = self.sess.array(np.ascontiguousarray(values.T)) if n else self.sess.array(shape=(4,))
        out = np.full((n_terms, max(n, 4)), -77.0, np.float32)
        d_t = self.sess.array(out)
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        try:
            self.sess.rdl.rdl_component_terms(
                self.sess.h, C.c_uint32(self.mode), C.c_uint32(self.n_ch), C.c_uint32(n_terms),
                ptr(self.map, C.c_double) if self.mode == POLYNOMIAL else None,
                ptr(self.fitted, C.c_uint8) if self.mode == POLYNOMIAL else None,
                None if self.lp is None else C.byref(self.lp),
                None if self.forced is None else C.byref(self.forced),
                C.c_uint32(width), C.c_uint32(height),
                None if xy is None else ptr(xy[0], C.c_uint32),
                None if xy is None else ptr(xy[1], C.c_uint32),
                d_v.vp if d_values else None, C.c_size_t(max(n, 1)), C.c_size_t(n), d_t.vp,
                C.c_size_t(max(n, 4)))
            self.sess.sync()
            return d_t.get()[:, :n].T if n else d_t.get()
        finally:
            self.last_output = d_t.get()
            d_v.free()
            d_t.free()

    def host(self, values, xy=None):
        out = np.empty((len(values), self.n_terms), np.float32)
        for i, v in enumerate(values):
            x, y = (0, 0) if xy is None else (int(xy[0, i]), int(xy[1, i]))
            out[i] = self.fitter.fit([float(t) for t in v], x, y)
        return out

    def evaluate(self, terms):
        """S at every channel from (n, n_terms) log-polynomial terms, float64"""
        lg = np.asarray([self.lp.lg[c] for c in range(self.n_ch)])[None, :]
        e = np.zeros((len(terms), self.n_ch))
        for k in range(self.n_terms - 1, 0, -1):
            e = (e + terms[:, k:k + 1].astype(np.float64)) * lg
        return terms[:, :1].astype(np.float64) * 10.0 ** e

    def free(self):
        if self.d_planes is not None:
            self.d_planes.free()


def check(case, values, got, xy=None, rows=None):
    """got (n, n_terms) from the device against the host fit of `rows`
    (every component when None)."""
    rows = np.arange(len(values)) if rows is None else rows
    values, got = values[rows], got[rows]
    xy = None if xy is None else xy[:, rows]
    assert np.all(np.isfinite(got))
    if case.mode == POLYNOMIAL:
        # the host map applied in float64 numpy, and the host fitter itself
        v = values.astype(np.float64) * case.fitted[None, :]
        want = v @ case.map.T
        bound = (2.0 ** -23 * np.abs(want) + 1e-12 * (np.abs(v) @ np.abs(case.map).T))
        err = np.abs(got.astype(np.float64) - want)
        print(f"polynomial: max |d| / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert np.all(err <= bound)
        few = slice(0, min(len(values), 300))
        host = case.host(values[few]).astype(np.float64)
        assert np.all(np.abs(got[few].astype(np.float64) - host) <= bound[few])
    elif case.mode == FORCED:
        host = case.host(values, xy)
        if case.n_terms > 1:
            planes = case.planes[:, xy[1], xy[0]].T
            assert np.array_equal(got[:, 1:].view(np.uint32), planes.view(np.uint32))
        ulp = np.spacing(np.abs(host[:, 0]).astype(np.float32)).astype(np.float64)
        err = np.abs(got[:, 0].astype(np.float64) - host[:, 0].astype(np.float64))
        print(f"forced: max t0 error = {np.max(err / ulp):.3g} ulp")
        assert np.all(err <= 2.0 * ulp)
    else:
        host = case.host(values)
        atol = 2e-5 * max(1.0, float(np.max(np.abs(host))))
        err = np.abs(got.astype(np.float64) - host.astype(np.float64))
        rel = err / (atol + 2e-5 * np.abs(host.astype(np.float64)))
        s_got, s_host = case.evaluate(got), case.evaluate(host)
        s_atol = 1e-6 * float(np.max(np.abs(values)))
        s_rel = np.abs(s_got - s_host) / (s_atol + 1e-4 * np.abs(s_host))
        print(f"log-polynomial {case.n_ch} ch {case.n_terms} terms: max term error / bound = "
              f"{np.max(rel):.3g}, max spectrum error / bound = {np.max(s_rel):.3g}, "
              f"bit-equal terms {np.mean(got.view(np.uint32) == host.view(np.uint32)):.4f}")
        np.testing.assert_allclose(got, host, rtol=2e-5, atol=atol)
        np.testing.assert_allclose(s_got, s_host, rtol=1e-4, atol=s_atol)


def run_case(sess, mode, n_ch, n_terms, n, zero=None, seed=0, sample=None, transform=None):
    case = Case(sess, mode, n_ch, n_terms, zero)
    try:
        rng = np.random.default_rng(1000 * mode + 100 * n_ch + 10 * n_terms + seed)
        values = spectra(rng, case.fitter, n)
        if transform is not None:
            values = transform(values)
        xy = case.positions(rng, n) if mode == FORCED else None
        got = case.device(values, xy)
        assert got.shape == (n, n_terms)
        rows = None
        if sample is not None and n > sample:
            rows = np.sort(np.random.default_rng(7).choice(n, sample, replace=False))
        check(case, values, got, xy, rows)
    finally:
        case.free()


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
@pytest.mark.parametrize("n", COUNTS)
def test_counts(sess, mode, n):
    run_case(sess, mode, 5, 3, n, zero=2)


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
def test_more_components_than_one_grid_round(sess, mode):
    # polynomial: all of them against the host map; the fits that loop in
    # Python on the host: a fixed random sample
    run_case(sess, mode, 5, 3, BIG, zero=2, sample=None if mode == POLYNOMIAL else SAMPLE)


SHAPES = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (5, 1), (5, 2), (5, 3), (16, 1), (16, 2),
          (16, 3), (16, 8)]


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
@pytest.mark.parametrize("n_ch,n_terms", SHAPES)
def test_shapes(sess, mode, n_ch, n_terms):
    run_case(sess, mode, n_ch, n_terms, 257, zero=1 if n_ch >= 5 else None)


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
def test_negative_spectra(sess, mode):
    run_case(sess, mode, 5, 3, 65, transform=lambda v: -v)


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
def test_zero_spectrum(sess, mode):
    def with_zeros(v):
        v[::3] = 0.0
        return v
    run_case(sess, mode, 5, 3, 65, transform=with_zeros)


def test_forced_corners(sess):
    case = Case(sess, FORCED, 5, 3)
    try:
        values = spectra(np.random.default_rng(3), case.fitter, 4)
        xy = np.ascontiguousarray(
            np.array([[0, W - 1, 0, W - 1], [0, 0, H - 1, H - 1]], np.uint32))
        check(case, values, case.device(values, xy), xy)
    finally:
        case.free()


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
def test_no_components(sess, mode):
    case = Case(sess, mode, 5, 3)
    try:
        xy = np.zeros((2, 1), np.uint32) if mode == FORCED else None
        out = case.device(np.zeros((0, 5), np.float32), xy)
        assert np.all(out == -77.0)
    finally:
        case.free()


def refused(case, **kwargs):
    values = spectra(np.random.default_rng(4), case.fitter, 8)
    xy = kwargs.pop("xy", case.positions(np.random.default_rng(4), 8)
                    if case.mode == FORCED else None)
    with pytest.raises(RdlError):
        case.device(values, xy, **kwargs)
    assert np.all(case.last_output == -77.0)  # nothing was launched


@pytest.mark.parametrize("mode", [POLYNOMIAL, LOGPOLY, FORCED])
def test_null_values_are_refused(sess, mode):
    case = Case(sess, mode, 5, 3)
    try:
        refused(case, d_values=False)
    finally:
        case.free()


@pytest.mark.parametrize("mode", [LOGPOLY, FORCED])
def test_nine_terms_are_refused(sess, mode):
    case = Case(sess, mode, 5, 3)
    try:
        case.lp.n_terms = 9
        refused(case, n_terms=9)
    finally:
        case.free()


def test_forced_component_outside_the_image_is_refused(sess):
    case = Case(sess, FORCED, 5, 3)
    try:
        xy = case.positions(np.random.default_rng(4), 8)
        xy[0, 5] = W  # x == width
        refused(case, xy=xy)
        xy[0, 5], xy[1, 7] = 0, H
        refused(case, xy=xy)
        # planes smaller than the image
        refused(case, width=W + 1)
    finally:
        case.free()
