"""Forced-term spectral fitting (spectral_fitting.mode = forced_terms,
WSClean's -force-spectrum): the shape terms t1, t2, ... of every component
come from term planes at its pixel and only the flux term is fitted,

    f_c = 10^(t1 lg_c + t2 lg_c^2 + ...),   lg_c = log10(nu_c / nu_ref)
    t0  = sum_c w_c v_c / sum_c w_c f_c     over the channels with w_c > 0
    fitted value of channel c = t0 f_c

(csrc/hip/logpoly.h; schaapcommon's fitter is not vendored: PARITY UNPINNED,
DESIGN.md). The oracle has no forced mode, so the expectations are this
closed form in numpy float64, and — with all-zero term planes, where the fit
is the weighted mean — the oracle's one-term polynomial run.

CPU: the host fitter against numpy. GPU: rdl_forced_interpolate against
numpy; the first component of Högbom / Clark / multiscale runs against the
closed form; zero planes against the oracle (trace, residual, model);
position-dependent planes: every model pixel's spectrum has its own pixel's
shape, on one image and on a 2 x 2 grid of subimages (which fails when a
subimage's origin inside the planes is dropped); Radler with a term cube on
disk and fewer deconvolution than original channels.
"""
import ctypes as C

import numpy as np
import pytest

from fits_helper import write_fits
from oracle_lib import OracleAlgorithm, get_oracle
from radler_import import radler as rd
from synthetic import problem

POLY = 1
FORCED = rd.SpectralFittingMode.forced_terms


class ForcedTerms(C.Structure):
    """rdl_forced_terms (include/rdl_hip.h): device term planes of a forced fit."""
    _fields_ = [("d_planes", C.c_void_p), ("plane_stride", C.c_size_t),
                ("pitch", C.c_uint32), ("rows", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32),
                ("weights", C.c_float * 16)]


def _reference_frequency(freqs, wts):
    f, w = np.asarray(freqs, np.float64), np.asarray(wts, np.float64)
    return np.sum(f * w) / np.sum(w) if np.sum(w) > 0 else np.mean(f)


def _shape(terms, lg):
    """f = 10^(sum_k terms[k-1] lg^k): terms (n_terms-1, ...), lg (n, 1...)."""
    e = np.zeros(np.broadcast(terms[0], lg).shape)
    for k in range(len(terms), 0, -1):
        e = (e + terms[k - 1]) * lg
    return 10.0 ** e


def _forced_fit(values, wts, shape):
    """t0 of float64 values / shape with a leading channel axis."""
    w = np.asarray(wts, np.float64).reshape((-1,) + (1,) * (values.ndim - 1))
    use = w > 0
    num = np.sum(np.where(use, w * values, 0.0), axis=0)
    den = np.sum(np.where(use, w * shape, 0.0), axis=0)
    return np.where(den != 0.0, num / np.where(den != 0.0, den, 1.0), 0.0)


# -------------------------------------------------------------------- host
@pytest.mark.parametrize("n_ch,n_terms", [(1, 2), (4, 2), (6, 3), (5, 4)])
def test_host_forced_fitter_matches_numpy(n_ch, n_terms):
    rng = np.random.default_rng(10 * n_ch + n_terms)
    w_px, h_px = 7, 5  # non-square planes
    freqs = 1.0e8 + 1.5e7 * np.arange(n_ch) + rng.uniform(0, 2e6, n_ch)
    wts = rng.uniform(0.5, 3.0, n_ch).astype(np.float32)
    if n_ch > 1:
        wts[1] = 0.0
    planes = [rng.uniform(-1.5, 1.0, (h_px, w_px)).astype(np.float32) / (k + 1)
              for k in range(n_terms - 1)]
    fitter = rd.SpectralFitter(FORCED, n_terms, list(freqs), list(wts))
    with pytest.raises(RuntimeError, match="term planes"):
        fitter.fit([1.0] * n_ch)  # no planes yet
    with pytest.raises(RuntimeError, match="term planes given"):
        fitter.set_forced_terms(planes + [planes[0]])
    fitter.set_forced_terms(planes)
    lg = np.log10(freqs / _reference_frequency(freqs, wts))
    for x, y in [(0, 0), (6, 4), (3, 1), (1, 3)]:
        v = rng.standard_normal(n_ch).astype(np.float32) + np.float32(2.0)
        terms = np.array([p[y, x] for p in planes], np.float64)
        shape = _shape(terms, lg)
        t0 = _forced_fit(v.astype(np.float64), wts, shape)
        exp = t0 * shape
        got = np.array(fitter.fit_and_evaluate(list(v), x, y), np.float32)
        np.testing.assert_allclose(got, exp, atol=2e-6 * max(1.0, float(np.abs(exp).max())))
        t = np.array(fitter.fit(list(v), x, y))
        assert t[0] == pytest.approx(float(t0), abs=2e-6 * max(1.0, abs(float(t0))))
        assert np.array_equal(t[1:].astype(np.float32), terms.astype(np.float32))
        # the weighted sum of the fit equals that of the data
        use = wts > 0
        assert np.sum(wts[use] * got[use]) == pytest.approx(np.sum(wts[use] * v[use]),
                                                            rel=1e-5, abs=1e-5)
    with pytest.raises(RuntimeError, match="outside"):
        fitter.fit([1.0] * n_ch, 7, 0)


def test_host_forced_fitter_zero_plane_is_weighted_mean_and_indexing():
    freqs, wts = [1.0e8, 1.2e8, 1.4e8], [1.0, 0.5, 2.0]
    fitter = rd.SpectralFitter(FORCED, 2, freqs, wts)
    fitter.set_forced_terms([np.zeros((5, 7), np.float32)])
    v = [1.0, 4.0, -2.5]
    mean = np.average(v, weights=wts)
    np.testing.assert_allclose(fitter.fit_and_evaluate(v, 2, 3), mean, rtol=1e-6)
    # a ramp plane: (x, y) and (y, x) are different pixels
    yy, xx = np.mgrid[0:5, 0:7]
    fitter.set_forced_terms([(0.1 * xx - 0.3 * yy).astype(np.float32)])
    a = fitter.fit_and_evaluate(v, 1, 3)
    b = fitter.fit_and_evaluate(v, 3, 1)
    assert not np.allclose(a, b, rtol=1e-3)
    assert fitter.fit(v, 1, 3)[1] == pytest.approx(0.1 * 1 - 0.3 * 3, rel=1e-6)
    assert fitter.fit(v, 3, 1)[1] == pytest.approx(0.1 * 3 - 0.3 * 1, rel=1e-6)
    # every weight zero, or a vanishing divisor: t0 = 0
    zero = rd.SpectralFitter(FORCED, 2, freqs, [0.0, 0.0, 0.0])
    zero.set_forced_terms([np.zeros((5, 7), np.float32)])
    assert zero.fit_and_evaluate(v, 0, 0) == [0.0, 0.0, 0.0]


# --------------------------------------------------------------------- GPU
def _compact_psf(w, h, fwhm=4.0, radius=10):
    """A Gaussian core cut off at `radius` pixels, so that the Högbom window,
    the padded FFT correction and a zero-filled shift agree away from the
    edges."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = (xx - w // 2) ** 2 + (yy - h // 2) ** 2
    psf = np.exp(-0.5 * r2 / (fwhm / 2.3548) ** 2) * (r2 <= radius * radius)
    return psf.astype(np.float32)


def _shift(psf, x0, y0):
    h, w = psf.shape
    out = np.zeros_like(psf)
    dx, dy = x0 - w // 2, y0 - h // 2
    ys, xs = slice(max(dy, 0), h + min(dy, 0)), slice(max(dx, 0), w + min(dx, 0))
    yd, xd = slice(max(-dy, 0), h + min(-dy, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    out[ys, xs] = psf[yd, xd]
    return out


def _planes(w, h):
    """T1 = -1 + 0.004 x + 0.01 y, T2 = 0.2 - 0.003 x."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([-1.0 + 0.004 * xx + 0.01 * yy, 0.2 - 0.003 * xx]).astype(np.float32)


VARIANTS = {"hogbom": (0, False), "clark": (0, True), "ms_fast": (1, True),
            "ms_slow": (1, False)}


def _settings(variant, w, h, terms, path, max_iter, thr):
    kind, flag = VARIANTS[variant]
    s = rd.Settings()
    s.trimmed_image_width, s.trimmed_image_height = w, h
    s.pixel_scale.x = s.pixel_scale.y = 1.0 / 3600.0 * np.pi / 180.0
    s.minor_iteration_count = max_iter
    s.absolute_threshold = thr
    s.border_ratio = 0.0
    s.spectral_fitting.mode = FORCED
    s.spectral_fitting.terms = terms
    s.spectral_fitting.forced_filename = path
    if kind == 1:
        s.algorithm_type = rd.AlgorithmType.multiscale
        s.multiscale.fast_sub_minor_loop = flag
    else:
        s.algorithm_type = rd.AlgorithmType.generic_clean
        s.generic.use_sub_minor_optimization = flag
    return s, kind


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out,terms,w,h", [(4, 10, 2, 96, 80), (3, 3, 3, 64, 33),
                                                   (8, 16, 2, 130, 70)])
def test_forced_interpolate_kernel_matches_numpy(n_in, n_out, terms, w, h):
    """rdl_forced_interpolate (ImageSet::InterpolateAndStoreModel in forced
    mode) against the definition in numpy float64; the planes are larger than
    the image and the image sits at an origin inside them."""
    from rdl_lib import Session, logpoly
    rng = np.random.default_rng(n_in + 10 * terms)
    f_in = 1.0e8 + 2.0e7 * np.arange(n_in)
    wts = rng.uniform(0.5, 2.0, n_in).astype(np.float32)
    wts[1] = 0.0  # a channel that is evaluated, not fitted
    ref = _reference_frequency(f_in, wts)
    x0, y0, pitch, rows = 3, 2, w + 5, h + 4
    full = np.stack([rng.uniform(-1.5, 0.5, (rows, pitch)) / (k + 1)
                     for k in range(terms - 1)]).astype(np.float32)
    amp = rng.standard_normal((h, w))
    lg = np.log10(f_in / ref)[:, None, None]
    planes = (amp * (1.0 + 0.2 * rng.standard_normal((n_in, h, w)))).astype(np.float32)
    planes[:, rng.random((h, w)) < 0.5] = 0.0  # zero pixels are not fitted
    f_out = np.linspace(f_in[0] - 5e6, f_in[-1] + 5e6, n_out)
    out_lg = np.log10(f_out / ref)
    lp = logpoly(f_in, wts, terms)
    sess = Session(0)
    try:
        d_in = sess.array(planes)
        d_terms = sess.array(full)
        d_out = sess.array(np.zeros((n_out, h, w), np.float32))
        ft = ForcedTerms()
        ft.d_planes, ft.plane_stride = d_terms.ptr, pitch * rows
        ft.pitch, ft.rows, ft.x0, ft.y0 = pitch, rows, x0, y0
        for c in range(n_in):
            ft.weights[c] = wts[c]
        args = [sess.h, d_in.vp, C.c_size_t(h * w), C.c_uint32(w), C.c_uint32(h), C.byref(lp),
                C.byref(ft), out_lg.ctypes.data_as(C.c_void_p), C.c_uint32(n_out), d_out.vp,
                C.c_size_t(h * w)]
        sess.rdl.rdl_forced_interpolate(*args)
        got = d_out.get()
        # planes that do not cover the image are refused before any launch
        ft.x0 = 6
        with pytest.raises(RuntimeError, match="do not cover"):
            sess.rdl.rdl_forced_interpolate(*args)
        for d in (d_in, d_terms, d_out):
            d.free()
    finally:
        sess.close()
    t = full[:, y0:y0 + h, x0:x0 + w].astype(np.float64)
    t0 = _forced_fit(planes.astype(np.float64), wts, _shape(t, lg))
    t0 = t0.astype(np.float32).astype(np.float64)  # the terms are float
    exp = t0 * _shape(t, out_lg[:, None, None])
    zero = np.all(planes == 0.0, axis=0)
    assert 0.3 < zero.mean() < 0.7
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-6 * np.abs(exp).max())
    assert np.all(got[:, zero] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["hogbom", "clark", "ms_fast", "ms_slow"])
def test_first_component_known_answer(tmp_path, variant):
    w, h, n_ch = 96, 80, 4
    wts = np.array([1.0, 0.5, 2.0, 1.0])
    x0, y0 = 50, 37
    flux = np.array([1.0, 0.8, 0.7, 0.45], np.float32)
    psf = _compact_psf(w, h)
    at = _shift(psf, x0, y0)
    dirty = (flux[:, None, None] * at[None]).astype(np.float32)
    planes = _planes(w, h)
    path = str(tmp_path / "terms.fits")
    write_fits(path, planes)
    s, kind = _settings(variant, w, h, 3, path, 1, 1e-3)
    if kind == 1:
        s.multiscale.max_scales = 1  # the delta scale only
    run = rd.gpu.DeviceRun(s, np.stack([psf] * n_ch), dirty, list(wts),
                           2.0 * s.pixel_scale.x if kind == 1 else 0.0)
    r = run.execute()
    assert r["iterations"] == 1
    assert [tuple(t[:2]) for t in run.trace()] == [(x0, y0)]
    freqs = 1.0e8 + 1.0e7 * np.arange(n_ch)  # DeviceRun's channel frequencies
    lg = np.log10(freqs / _reference_frequency(freqs, wts))
    shape = _shape(planes[:, y0, x0].astype(np.float64), lg)
    gain = 0.1
    value = gain * _forced_fit(flux.astype(np.float64), wts, shape) * shape
    model = run.model().reshape(n_ch, h, w)
    tol = 2e-5 * np.abs(dirty).max()
    expect = np.zeros_like(model)
    expect[:, y0, x0] = value
    print("model", model[:, y0, x0], "expected", value)
    np.testing.assert_allclose(model[:, y0, x0], value, atol=tol)
    assert np.count_nonzero(model) == n_ch and np.array_equal(model != 0, expect != 0)
    residual = run.residual().reshape(n_ch, h, w)
    np.testing.assert_allclose(residual, dirty - value[:, None, None] * at[None], atol=tol)


def _joined(w, n_ch, seed):
    """tests/test_spectral.py's joined-channel problem."""
    psf, dirty = problem(w, w, 14, 3, seed=seed)
    rng = np.random.default_rng(seed)
    dirties = np.stack([dirty * np.float32(1.0 + 0.15 * k) + np.float32(2e-3) *
                        rng.standard_normal((w, w)).astype(np.float32)
                        for k in range(n_ch)]).astype(np.float32)
    return np.stack([psf] * n_ch), dirties


@pytest.mark.gpu
@pytest.mark.parametrize("variant,n_ch,weights", [
    ("clark", 4, None), ("hogbom", 3, [1.0, 2.0, 0.5]), ("ms_fast", 4, [1.0, 0.5, 2.0, 1.0])])
def test_zero_planes_equal_one_term_polynomial(tmp_path, variant, n_ch, weights):
    """With all-zero term planes the forced fit is the weighted channel mean,
    which is the oracle's one-term polynomial fit."""
    kind = VARIANTS[variant][0]
    w, terms = (128 if kind == 1 else 96), 2
    psfs, dirties = _joined(w, n_ch, 40 + n_ch + terms)
    wts = np.ones(n_ch) if weights is None else np.asarray(weights, np.float64)
    freqs = 1.0e8 + 1.0e7 * np.arange(n_ch)
    thr, max_iter = 1.2e-2, 400
    st = dict(threshold=thr, max_iterations=max_iter, border_ratio=0.0)
    if kind == 1:
        st.update(max_scales=3, beam_size_in_pixels=2.0, fast_sub_minor_loop=1)
    else:
        st.update(use_sub_minor=int(variant == "clark"))
    orc = get_oracle()
    orc.set_threads(8)
    alg = OracleAlgorithm(orc, kind, **st)
    alg.set_spectral_fitter(POLY, 1, freqs, wts)
    res_o, mod_o = dirties.copy(), np.zeros_like(dirties)
    r_o, trace_o = alg.execute(res_o, mod_o, psfs, weights=wts.astype(np.float32))

    path = str(tmp_path / "zero.fits")
    write_fits(path, np.zeros((1, w, w), np.float32))
    s, _ = _settings(variant, w, w, terms, path, max_iter, thr)
    if kind == 1:
        s.multiscale.max_scales = 3
    run = rd.gpu.DeviceRun(s, psfs, dirties, list(wts),
                           2.0 * s.pixel_scale.x if kind == 1 else 0.0)
    r_g = run.execute()
    t_g = run.trace() if kind == 1 else run.trace()[:, :2]
    t_o = trace_o if kind == 1 else trace_o[:, :2]
    n = min(len(t_g), len(t_o))
    differ = np.nonzero(np.any(t_g[:n] != t_o[:n], axis=1))[0]
    if len(differ):
        print("traces differ first at step", differ[0], t_g[differ[0]], t_o[differ[0]])
    assert r_g["iterations"] == r_o.iteration_number > 10
    assert np.array_equal(t_g, t_o)
    tol = 2e-5 * np.abs(dirties).max()
    np.testing.assert_allclose(run.residual().reshape(n_ch, w, w), res_o, atol=tol)
    np.testing.assert_allclose(run.model().reshape(n_ch, w, w), mod_o, atol=tol)


def _sources(w, h, n, seed, margin=14):
    """Point sources on a jittered grid, at least 12 pixels apart, with
    falling spectra."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cell_x, cell_y = (w - 2 * margin) / side, (h - 2 * margin) / side
    out = []
    for i in range(n):
        cx = margin + (i % side + 0.5) * cell_x + rng.uniform(-1, 1)
        cy = margin + (i // side + 0.5) * cell_y + rng.uniform(-1, 1)
        out.append((int(round(cx)), int(round(cy)), rng.uniform(0.5, 1.0),
                    rng.uniform(-1.2, -0.2)))
    return out


def _sky(w, h, n_ch, sources, psf):
    freqs = 1.0e8 + 1.0e7 * np.arange(n_ch)
    dirty = np.zeros((n_ch, h, w), np.float64)
    for x, y, flux, alpha in sources:
        at = _shift(psf, x, y)
        for c in range(n_ch):
            dirty[c] += flux * (freqs[c] / freqs[0]) ** alpha * at
    return dirty.astype(np.float32)


def _check_shapes(model, planes, wts, min_pixels):
    """model[:, y, x] / f(x, y) is constant over channels at every non-zero
    pixel: every component at a pixel has that pixel's terms."""
    n_ch = model.shape[0]
    freqs = 1.0e8 + 1.0e7 * np.arange(n_ch)
    lg = np.log10(freqs / _reference_frequency(freqs, wts))[:, None]
    ys, xs = np.nonzero(np.any(model != 0.0, axis=0))
    assert len(ys) >= min_pixels, len(ys)
    shape = _shape(planes[:, ys, xs].astype(np.float64), lg)
    ratio = model[:, ys, xs].astype(np.float64) / shape
    spread = np.abs(ratio - ratio.mean(axis=0)).max(axis=0) / np.abs(ratio).max(axis=0)
    print("non-zero pixels", len(ys), "largest relative spread", spread.max())
    assert spread.max() <= 1e-5
    return ys, xs


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["hogbom", "clark"])
def test_components_take_the_shape_of_their_pixel(tmp_path, variant):
    w = h = 96
    n_ch, wts = 4, [1.0, 0.5, 2.0, 1.0]
    psf = _compact_psf(w, h)
    dirty = _sky(w, h, n_ch, _sources(w, h, 25, 7), psf)
    planes = _planes(w, h)
    path = str(tmp_path / "terms.fits")
    write_fits(path, planes)
    s, _ = _settings(variant, w, h, 3, path, 200, 1e-4)
    run = rd.gpu.DeviceRun(s, np.stack([psf] * n_ch), dirty, wts, 0.0)
    r = run.execute()
    assert r["iterations"] == 200
    _check_shapes(run.model().reshape(n_ch, h, w), planes, wts, 20)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["hogbom", "clark"])
def test_tiled_run_uses_the_full_image_planes(tmp_path, variant):
    """A 2 x 2 grid of subimages: every subimage's loop must read the terms
    at its origin inside the full planes."""
    w = h = 128
    n_ch, wts = 4, [1.0, 0.5, 2.0, 1.0]
    psf = _compact_psf(w, h)
    dirty = _sky(w, h, n_ch, _sources(w, h, 36, 11), psf)
    planes = _planes(w, h)
    path = str(tmp_path / "terms.fits")
    write_fits(path, planes)
    s, _ = _settings(variant, w, h, 3, path, 200, 1e-4)
    s.parallel.grid_width = s.parallel.grid_height = 2
    s.parallel.max_threads = 2
    run = rd.gpu.DeviceRun(s, np.stack([psf] * n_ch), dirty, wts, 0.0)
    r = run.execute()
    assert r["iterations"] > 100
    model = run.model().reshape(n_ch, h, w)
    ys, xs = _check_shapes(model, planes, wts, 20)
    for qy in (ys < h // 2, ys >= h // 2):
        for qx in (xs < w // 2, xs >= w // 2):
            assert np.count_nonzero(qy & qx) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", [rd.AlgorithmType.generic_clean,
                                       rd.AlgorithmType.multiscale])
def test_radler_with_a_term_cube_on_disk(tmp_path, algorithm):
    """Two deconvolution channels of four original ones: the stored models
    follow t0(x, y) 10^(T1(x, y) lg_g) at the original frequencies."""
    w, h, n_orig = 64, 48, 4
    psf = _compact_psf(w, h)
    sources = [(x, y, fl, a) for x, y, fl, a in _sources(w, h, 6, 3, margin=12)]
    freqs = 1.0e8 + 1.0e7 * np.arange(n_orig)
    residuals = _sky(w, h, n_orig, sources, psf)
    models = np.zeros_like(residuals)
    psfs = np.stack([psf] * n_orig)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    t1 = (-1.0 + 0.01 * xx + 0.02 * yy).astype(np.float32)
    s = rd.Settings()
    s.algorithm_type = algorithm
    s.trimmed_image_width, s.trimmed_image_height = w, h
    s.pixel_scale.x = s.pixel_scale.y = 1.0 / 3600.0 * np.pi / 180.0
    s.minor_iteration_count = 600
    s.absolute_threshold = 1e-2
    s.border_ratio = 0.0
    s.multiscale.max_scales = 1
    s.spectral_fitting.mode = FORCED
    s.spectral_fitting.terms = 2
    s.spectral_fitting.forced_filename = str(tmp_path / "terms.fits")
    write_fits(s.spectral_fitting.forced_filename, t1[None])
    bands = np.stack([freqs - 5e6, freqs + 5e6], axis=1)
    wts = np.array([1.0, 0.5, 2.0, 1.0])
    r = rd.Radler(s, psfs, residuals, models, 2.0 * s.pixel_scale.x, 2, bands, wts)
    r.perform(0)
    assert r.iteration_number > 20
    ys, xs = np.nonzero(np.any(models != 0.0, axis=0))
    assert len(ys) >= len(sources)
    # lg relative to any reference: a change of reference scales every
    # channel of a pixel by one factor, which the fitted amplitude absorbs
    lg = np.log10(freqs / freqs.mean())[:, None]
    shape = 10.0 ** (t1[ys, xs].astype(np.float64) * lg)
    spectra = models[:, ys, xs].astype(np.float64)
    amplitude = (spectra / shape).mean(axis=0)
    tol = 2e-5 * np.abs(models).max()
    print("largest deviation", np.abs(spectra - amplitude * shape).max(), "tolerance", tol)
    np.testing.assert_allclose(spectra, amplitude * shape, atol=tol)
    # the sources were cleaned: the integrated residual fell to the threshold
    # (the forced shapes are not the sources' own, so single channels keep some)
    assert np.abs(np.average(residuals, axis=0, weights=wts)).max() < 0.05
